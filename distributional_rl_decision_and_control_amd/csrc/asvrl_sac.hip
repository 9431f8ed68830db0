// asvrl_sac.hip -- SAC (agent.py:289-306 act_sac, 547-595 train_SAC) on MFMA (gfx950). SAC_model.Critic is
// DDPG_model.Critic line for line: the twin critics run the one-scalar critic tile of asvrl_ddpg_tile.h unchanged.
// SAC_model.Actor is the Actor's trunk (trunk_chain, asvrl_actor_tile.h) under two 128 -> 2 heads: four f32 dot
// products per row closed by one exchange between the lane halves, then the reparameterised sample, the atan squash
// and the log-probability per lane. Every kernel runs the one-wave 32-row Actor tile, 4 waves per workgroup.
//
// Kernels:
//   sac_act_kernel          act_sac on n robot rows: the sampled action under the epsilon schedule (atile::explore)
//   sac_actor_fwd_kernel    blockIdx.y = 0 the local actor on s saving xb / h0 / h1 / h2 and the head's values;
//                           1 the target actor on s' -> na, logp_next
//   sac_fwd_kernel          the critic update's four forwards: blockIdx.y = 0, 1 local 1, 2 on (s, a) saving the
//                           activations; 2, 3 target 1, 2 on (s', na)
//   sac_bwd_kernel          blockIdx.y = k: y = r + gamma (1 - d) (min q_next - alpha logp_next), MSE loss partials,
//                           dq_k and critic k's backward (ddpg_bwd_tile)
//   sac_actor_q_kernel      blockIdx.y = k, through the updated critics. <false>: Q_k(s, a_pi). <true>, a second
//                           launch that reads both: w_k d(-Q_k)/da, w_k = 1 / 0.5 / 0 by torch.min's gradient rule
//                           (two critics' images do not fit in one workgroup's LDS together)
//   sac_actor_bwd_kernel    the head's backward, dz2, dz1, dz0 and the actor-loss partials; no LDS, no barrier
// Noise: eps given by the caller is used as is; otherwise Philox-4x32-10 + Box-Muller keyed by (row, counter, seed)
// with one domain constant per stream, so that two streams never share draws. The eps used is written out.
#include "asvrl_common.h"
#include "asvrl_mfma.h"
#include "asvrl_lds.h"
#include "asvrl_actor_tile.h"
#include "asvrl_ddpg_tile.h"
#include "asvrl_sac_tile.h"

namespace asvrl {
namespace {
using namespace atile;
using namespace ddtile;
using namespace sactile;   // the head, its noise and its sample: asvrl_sac_tile.h

constexpr int kSacWaves = 4;
constexpr int kSacT = kSacWaves * 64;
static_assert(sizeof(ActorLds) + sizeof(AeLds) <= 160 * 1024, "a critic's images and its action encoder in one CU's LDS");

// ------------------------------------------------------------------ act
struct SacActArgs {
  AsvSacActorWeights w;
  AsvSacActIO io;
};

__global__ __launch_bounds__(kSacT) void sac_act_kernel(SacActArgs a) {
  __shared__ ActorLds L;
  __shared__ SacHeadLds H;
  const AsvSacActIO& io = a.io;
  const int tile = blockIdx.x * kSacWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool active = tile * 32 < io.n;
  const int row = tile * 32 + (lane & 31);
  const bool valid = active && row < io.n;
  const int64_t rr = valid ? row : io.n - 1;
  frag8 bx[2];
  float mk[kObjN];
  if (active) load_obs(io.x, io.ldx, static_cast<int>(rr), lane >> 5, bx, mk);
  stage_actor<kSacT>(L, a.w.trunk, threadIdx.x);
  stage_head<kSacT>(H, a.w, threadIdx.x);
  __syncthreads();   // the only barrier: before any wave leaves
  if (!active) return;
  float h2v[8][8];
  trunk_chain<MLP_ACT>(a.w.trunk, AsvMlpIO{}, L, row, valid, lane, bx, mk, h2v);
  const uint64_t step = io.step_dev != nullptr ? static_cast<uint64_t>(*io.step_dev) : 0ull;
  float eps[kNa];
  if (io.eps_in != nullptr) {
    eps[0] = io.eps_in[2 * rr];
    eps[1] = io.eps_in[2 * rr + 1];
  } else {
    sac_eps(kSacActStream, static_cast<int>(rr), step, io.seed, eps[0], eps[1]);
  }
  SacSample o;
  sac_head(H, a.w.trunk.out_scale, h2v, lane, eps, o);
  if (!valid || (lane >> 5) != 0) return;
  io.eps_out[2 * rr] = eps[0];
  io.eps_out[2 * rr + 1] = eps[1];
  double* out = io.a_out64 + rr * 2;
  explore(step, EpsSchedule{io.eps_steps_per_count, io.eps_total, io.eps_fraction, io.eps_initial, io.eps_final},
          io.seed, row, o.a[0], o.a[1], out[0], out[1]);
}

// ------------------------------------------------------------------ actor forward (local on s, target on s')
struct SacActorFwdArgs {
  AsvSacActorWeights local, target;
  AsvSacActorIO io;
};

__global__ __launch_bounds__(kSacT) void sac_actor_fwd_kernel(SacActorFwdArgs a) {
  __shared__ ActorLds L;
  __shared__ SacHeadLds H;
  const AsvSacActorIO& io = a.io;
  const bool tgt = blockIdx.y != 0;   // workgroup-uniform
  const AsvSacActorWeights& w = tgt ? a.target : a.local;
  const int tile = blockIdx.x * kSacWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool active = tile * 32 < io.B;
  const int h = lane >> 5;
  const int row = tile * 32 + (lane & 31);
  const bool valid = active && row < io.B;
  const int64_t rr = valid ? row : io.B - 1;
  frag8 bx[2];
  float mk[kObjN];
  if (active) load_obs(io.rows + (tgt ? ASVRL_OBS_DIM : 0), io.ld_rows, static_cast<int>(rr), h, bx, mk);
  stage_actor<kSacT>(L, w.trunk, threadIdx.x);
  stage_head<kSacT>(H, w, threadIdx.x);
  __syncthreads();   // the only barrier: before any wave leaves
  if (!active) return;
  float h2v[8][8];
  if (tgt) {
    trunk_chain<MLP_FWD>(w.trunk, AsvMlpIO{}, L, row, valid, lane, bx, mk, h2v);
  } else {
    if (valid) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        *reinterpret_cast<frag8*>(bp(io.xb) + rr * kObsK + ks * 16 + 8 * h) = bx[ks];
    }
    AsvMlpIO mio = {};
    mio.h0 = io.h0;
    mio.h1 = io.h1;
    mio.h2 = io.h2;
    trunk_chain<MLP_TRAIN>(w.trunk, mio, L, row, valid, lane, bx, mk, h2v);
  }
  const uint64_t ctr = io.counter + (io.counter_dev != nullptr ? static_cast<uint64_t>(*io.counter_dev) : 0ull);
  const float* eps_in = tgt ? io.eps_target_in : io.eps_local_in;
  float eps[kNa];
  if (eps_in != nullptr) {
    eps[0] = eps_in[2 * rr];
    eps[1] = eps_in[2 * rr + 1];
  } else {
    sac_eps(tgt ? kSacTargetStream : kSacLocalStream, static_cast<int>(rr), ctr, io.seed, eps[0], eps[1]);
  }
  SacSample o;
  sac_head(H, w.trunk.out_scale, h2v, lane, eps, o);
  if (!valid || h != 0) return;
  if (tgt) {
    io.logp_next[rr] = o.logp;
#pragma unroll
    for (int d = 0; d < kNa; ++d) {
      io.na[2 * rr + d] = o.a[d];
      io.eps_next[2 * rr + d] = eps[d];
    }
  } else {
    io.logp[rr] = o.logp;
#pragma unroll
    for (int d = 0; d < kNa; ++d) {
      io.mu[2 * rr + d] = o.mu[d];
      io.ls[2 * rr + d] = o.ls[d];
      io.sigma[2 * rr + d] = o.sigma[d];
      io.z[2 * rr + d] = o.z[d];
      io.a[2 * rr + d] = o.a[d];
      io.eps[2 * rr + d] = eps[d];
    }
  }
}

// ------------------------------------------------------------------ twin critics: forwards
struct SacFwdArgs {
  AsvDdpgWeights net[4];   // local 1, local 2, target 1, target 2
  AsvSacGradIO io;
};

__global__ __launch_bounds__(kSacT) void sac_fwd_kernel(SacFwdArgs a) {
  __shared__ ActorLds L;
  __shared__ AeLds A;
  const bool tgt = blockIdx.y >= 2;   // workgroup-uniform
  const AsvDdpgWeights& w = a.net[blockIdx.y];
  const AsvDdpgGradIO& io = a.io.c[blockIdx.y & 1];
  const int tile = blockIdx.x * kSacWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool active = tile * 32 < io.B;
  const float* x = io.rows + (tgt ? ASVRL_OBS_DIM : 0);
  frag8 bx[2];
  float mk[kObjN];
  const int row = tile * 32 + (lane & 31);
  const bool valid = active && row < io.B;
  const int64_t rr = valid ? row : io.B - 1;
  float a0 = 0.f, a1 = 0.f;
  if (active) {
    load_obs(x, io.ld_rows, static_cast<int>(rr), lane >> 5, bx, mk);
    const float* ap = tgt ? io.na + rr * io.ld_na : io.rows + rr * io.ld_rows + kActCol;
    a0 = ap[0];
    a1 = ap[1];
  }
  stage_actor<kSacT>(L, w.trunk, threadIdx.x);
  stage_ae<kSacT>(A, w, threadIdx.x);
  __syncthreads();   // the only barrier: before any wave leaves
  if (!active) return;
  if (tgt) {
    const float q = ddpg_q_tile<DD_FWD>(w.trunk, io, L, A, row, valid, lane, bx, mk, a0, a1);
    if (valid && lane < 32) io.q_next[row] = q;
  } else {
    const float q = ddpg_q_tile<DD_TRAIN>(w.trunk, io, L, A, row, valid, lane, bx, mk, a0, a1);
    if (valid && lane < 32) io.q[row] = q;
  }
}

// ------------------------------------------------------------------ twin critics: target, MSE, backward
struct SacBwdArgs {
  AsvDdpgWeights local[2];
  AsvSacGradIO io;
};

__global__ __launch_bounds__(kSacT) void sac_bwd_kernel(SacBwdArgs a) {
  const int k = blockIdx.y;
  const AsvDdpgGradIO& io = a.io.c[k];
  const int tile = blockIdx.x * kSacWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile * 32 >= io.B) return;   // whole waves; the kernel has no barrier
  const int h = lane >> 5, r = lane & 31;
  const int row = tile * 32 + r;
  const bool valid = row < io.B;
  const int64_t rr = valid ? row : io.B - 1;
  // ---------------- target, loss and dq (agent.py:556-568)
  const float* rp = io.rows + rr * io.ld_rows + kActCol;
  const float a0 = rp[0], a1 = rp[1], rew = rp[2], done = rp[3];
  const float tv = fminf(a.io.c[0].q_next[rr], a.io.c[1].q_next[rr]) - a.io.alpha * a.io.logp_next[rr];
  const float y = rew + io.gamma * tv * (1.f - done);
  const float diff = io.q[rr] - y;
  const float inv_b = 1.f / static_cast<float>(io.B);
  float lossv = (valid && h == 0) ? diff * diff * inv_b : 0.f;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossv += __shfl_xor(lossv, off, 64);
  if (lane == 0) io.tile_loss[tile] = lossv;
  const float dq = valid ? 2.f * diff * inv_b : 0.f;
  if (valid && h == 0) {
    io.dq[row] = dq;
    if (k == 0 && a.io.y != nullptr) a.io.y[row] = y;
  }
  ddpg_bwd_tile(a.local[k], io, lane, rr, valid, a0, a1, dq);
}

// ------------------------------------------------------------------ actor step: Q_k(s, a_pi) and dA
struct SacActorGradArgs {
  AsvDdpgWeights local[2];
  AsvSacActorGradIO io;
};

template <bool BWD>
__global__ __launch_bounds__(kSacT) void sac_actor_q_kernel(SacActorGradArgs a) {
  __shared__ ActorLds L;
  __shared__ AeLds A;
  const AsvSacActorGradIO& io = a.io;
  const int k = blockIdx.y;   // workgroup-uniform
  const AsvDdpgWeights& w = a.local[k];
  const int tile = blockIdx.x * kSacWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool active = tile * 32 < io.B;
  frag8 bx[2];
  float mk[kObjN];
  const int row = tile * 32 + (lane & 31);
  const bool valid = active && row < io.B;
  const int64_t rr = valid ? row : io.B - 1;
  float a0 = 0.f, a1 = 0.f;
  if (active) {
    load_obs(io.x, io.ldx, static_cast<int>(rr), lane >> 5, bx, mk);
    a0 = io.act[rr * io.lda];
    a1 = io.act[rr * io.lda + 1];
  }
  stage_actor<kSacT>(L, w.trunk, threadIdx.x);
  stage_ae<kSacT>(A, w, threadIdx.x);
  __syncthreads();   // the only barrier: before any wave leaves
  if (!active) return;
  if constexpr (!BWD) {
    const float q = ddpg_q_tile<DD_FWD>(w.trunk, AsvDdpgGradIO{}, L, A, row, valid, lane, bx, mk, a0, a1);
    if (valid && lane < 32) io.q_pi[static_cast<int64_t>(k) * io.B + row] = q;
  } else {
    // d(-min(Q1, Q2))/dQ_k: -1 where Q_k is the smaller, -1/2 each on an exact tie (torch.min's backward), else 0
    const float mine = io.q_pi[static_cast<int64_t>(k) * io.B + rr];
    const float other = io.q_pi[static_cast<int64_t>(1 - k) * io.B + rr];
    const float dq = mine < other ? -1.f : (mine == other ? -0.5f : 0.f);
    ActorKeep keep;
    ddpg_q_tile<DD_ACTOR>(w.trunk, AsvDdpgGradIO{}, L, A, row, valid, lane, bx, mk, a0, a1, dq, &keep);
    float d0, d1;
    ddpg_dA_tile(w, A, keep, lane, d0, d1);
    if (valid && lane < 32) {
      float* o = io.dA + (static_cast<int64_t>(k) * io.B + rr) * 2;
      o[0] = d0;
      o[1] = d1;
    }
  }
}

// ------------------------------------------------------------------ actor backward
struct SacActorBwdArgs {
  AsvSacActorWeights w;
  AsvSacActorIO io;
};

__global__ __launch_bounds__(kSacT) void sac_actor_bwd_kernel(SacActorBwdArgs a) {
  const AsvSacActorIO& io = a.io;
  const int tile = blockIdx.x * kSacWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile * 32 >= io.B) return;   // whole waves; the kernel has no barrier
  const int h = lane >> 5, r = lane & 31;
  const int row = tile * 32 + r;
  const bool valid = row < io.B;
  const int64_t rr = valid ? row : io.B - 1;
  const int64_t B = io.B;
  const float g = 1.f / static_cast<float>(io.B), alpha = io.alpha;
  // ---------------- loss = mean(alpha logp - min(Q1, Q2)) (agent.py:585-587)
  const float qmin = fminf(io.q_pi[rr], io.q_pi[B + rr]);
  float lossv = (valid && h == 0) ? (alpha * io.logp[rr] - qmin) * g : 0.f;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossv += __shfl_xor(lossv, off, 64);
  if (lane == 0) io.tile_loss[tile] = lossv;
  // ---------------- the head: dL/da -> dL/dz -> dmu, dls
  float dh[kNHead];
#pragma unroll
  for (int d = 0; d < kNa; ++d) {
    const float av = io.a[2 * rr + d], z = io.z[2 * rr + d], e = io.eps[2 * rr + d];
    const float sg = io.sigma[2 * rr + d], ls = io.ls[2 * rr + d];
    const float dA = io.dA[2 * rr + d] + io.dA[2 * (B + rr) + d];   // d(-Qmin)/da, both critics' shares
    const float dLda = dA * g + (alpha * g) * (2.f * av) / ((1.f - av * av) + kMinVal);
    const float dLdz = dLda * (a.w.trunk.out_scale / (1.f + z * z));
    dh[d] = valid ? dLdz : 0.f;
    // z = mu + exp(ls) eps and the -ls term of logp; the clamp passes the gradient inside [-20, 2] only
    dh[kNa + d] = (valid && ls >= kLsMin && ls <= kLsMax) ? dLdz * e * sg - alpha * g : 0.f;
  }
  if (valid && h == 0) {
#pragma unroll
    for (int k = 0; k < kNHead; ++k) io.dhead[k * B + row] = dh[k];
  }
  // ---------------- dz2 = (Wmu^T dmu + Wls^T dls) 1[z2 > 0]
  const float* wh = a.w.head;
  frag8 dz2pk[8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    float hv[16];
    ddpg_load16(bp(io.h2) + rr * kHid, mb, h, hv);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = feat(mb, 8 * s + j, h);
        const float d = (wh[m] * dh[0] + wh[kHid + m] * dh[1]) + (wh[2 * kHid + m] * dh[2] + wh[3 * kHid + m] * dh[3]);
        dv[j] = hv[8 * s + j] > 0.f ? d : 0.f;
      }
      dz2pk[mb * 2 + s] = pack8(dv);
      store16(valid ? bp(io.dz2) + rr * kHid + mb * 32 + 16 * s : nullptr, dv, h);
    }
  }
  // ---------------- dz1 = (W2^T dz2) 1[z1 > 0]
  const frag8* W2T = reinterpret_cast<const frag8*>(a.w.trunk.w2t_frag);
  const frag8* W1T = reinterpret_cast<const frag8*>(a.w.trunk.w1t_frag);
  frag8 dz1pk[8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    float hv[16];
    ddpg_load16(bp(io.h1) + rr * kHid, mb, h, hv);
    f32x16 acc = f32x16{};
#pragma unroll
    for (int ks = 0; ks < kHid / 16; ++ks) acc = mfma(W2T[(mb * 8 + ks) * 64 + lane], dz2pk[ks], acc);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dv[j] = hv[8 * s + j] > 0.f ? acc[8 * s + j] : 0.f;
      dz1pk[mb * 2 + s] = pack8(dv);
      store16(valid ? bp(io.dz1) + rr * kHid + mb * 32 + 16 * s : nullptr, dv, h);
    }
  }
  // ---------------- dz0 = (W1^T dz1) 1[h0 > 0] (a masked object's feature is 0: no gradient reaches it)
#pragma unroll
  for (int mb = 0; mb < 8; ++mb) {
    float hv[16];
    ddpg_load16(bp(io.h0) + rr * kEnc, mb, h, hv);
    f32x16 acc = f32x16{};
#pragma unroll
    for (int ks = 0; ks < kHid / 16; ++ks) acc = mfma(W1T[(mb * 8 + ks) * 64 + lane], dz1pk[ks], acc);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dv[j] = hv[8 * s + j] > 0.f ? acc[8 * s + j] : 0.f;
      store16(valid ? bp(io.dz0) + rr * kEnc + mb * 32 + 16 * s : nullptr, dv, h);
    }
  }
}

// ------------------------------------------------------------------ argument checks
int sac_check_actor(const std::string& who, const char* name, const AsvSacActorWeights* w, bool backward) {
  ASVRL_REQUIRE(w != nullptr, who + ": null struct " + name);
  const std::string pre = who + ": null array " + name + ".";
#define ASVRL_SAC_W(field, ptr) ASVRL_REQUIRE((ptr) != nullptr, pre + field)
  if (backward) {
    ASVRL_SAC_W("w2t_frag", w->trunk.w2t_frag);
    ASVRL_SAC_W("w1t_frag", w->trunk.w1t_frag);
  } else {
    ASVRL_SAC_W("enc_frag", w->trunk.enc_frag);
    ASVRL_SAC_W("b_enc", w->trunk.b_enc);
    ASVRL_SAC_W("w1_frag", w->trunk.w1_frag);
    ASVRL_SAC_W("w2_frag", w->trunk.w2_frag);
    ASVRL_SAC_W("b1", w->trunk.b1);
    ASVRL_SAC_W("b2", w->trunk.b2);
    ASVRL_SAC_W("wout", w->trunk.wout);
    ASVRL_SAC_W("bout", w->trunk.bout);
    ASVRL_SAC_W("bhead", w->bhead);
  }
  ASVRL_SAC_W("head", w->head);
#undef ASVRL_SAC_W
  return 0;
}

int sac_check_rows(const std::string& who, const char* name, const float* rows, int64_t ld, int32_t B, int min_ld) {
  ASVRL_REQUIRE(rows != nullptr, who + ": null array " + name);
  ASVRL_REQUIRE(B >= 1 && B % 32 == 0, who + ": B must be a positive multiple of 32");
  ASVRL_REQUIRE(ld >= min_ld && ld % 4 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0,
                who + ": " + name + " must be 16-byte aligned rows");
  return 0;
}

int sac_groups(int32_t B) { return (B / 32 + kSacWaves - 1) / kSacWaves; }

}  // namespace
}  // namespace asvrl

using namespace asvrl;

extern "C" int64_t asvrl_sac_actor_weights_struct_size(void) { return sizeof(AsvSacActorWeights); }
extern "C" int64_t asvrl_sac_act_struct_size(void) { return sizeof(AsvSacActIO); }
extern "C" int64_t asvrl_sac_actor_struct_size(void) { return sizeof(AsvSacActorIO); }
extern "C" int64_t asvrl_sac_grad_struct_size(void) { return sizeof(AsvSacGradIO); }
extern "C" int64_t asvrl_sac_actor_grad_struct_size(void) { return sizeof(AsvSacActorGradIO); }

#define ASVRL_SAC_ARRAY(name) ASVRL_REQUIRE(io->name != nullptr, who + ": null array " #name)

extern "C" int asvrl_sac_act(const AsvSacActorWeights* w, const AsvSacActIO* io, void* stream) {
  const std::string who = "asvrl_sac_act";
  if (int rc = sac_check_actor(who, "w", w, false)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
  ASVRL_SAC_ARRAY(x);
  ASVRL_SAC_ARRAY(a_out64);
  ASVRL_SAC_ARRAY(eps_out);
  ASVRL_REQUIRE(io->n >= 1, who + ": n must be positive");
  ASVRL_REQUIRE(io->ldx >= ASVRL_OBS_DIM && io->ldx % 4 == 0 && reinterpret_cast<uintptr_t>(io->x) % 16 == 0,
                who + ": x must be 16-byte aligned rows");
  const int tiles = (io->n + 31) / 32;
  hipLaunchKernelGGL(sac_act_kernel, dim3((tiles + kSacWaves - 1) / kSacWaves), dim3(kSacT), 0, as_stream(stream),
                     SacActArgs{*w, *io});
  return check_launch("asvrl_sac_act");
}

extern "C" int asvrl_sac_actor_forward(const AsvSacActorWeights* local, const AsvSacActorWeights* target,
                                       const AsvSacActorIO* io, void* stream) {
  const std::string who = "asvrl_sac_actor_forward";
  if (int rc = sac_check_actor(who, "local", local, false)) return rc;
  if (int rc = sac_check_actor(who, "target", target, false)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
  if (int rc = sac_check_rows(who, "rows", io->rows, io->ld_rows, io->B, ASVRL_TR_DIM)) return rc;
  ASVRL_SAC_ARRAY(xb);
  ASVRL_SAC_ARRAY(h0);
  ASVRL_SAC_ARRAY(h1);
  ASVRL_SAC_ARRAY(h2);
  ASVRL_SAC_ARRAY(mu);
  ASVRL_SAC_ARRAY(ls);
  ASVRL_SAC_ARRAY(sigma);
  ASVRL_SAC_ARRAY(z);
  ASVRL_SAC_ARRAY(a);
  ASVRL_SAC_ARRAY(eps);
  ASVRL_SAC_ARRAY(logp);
  ASVRL_SAC_ARRAY(na);
  ASVRL_SAC_ARRAY(logp_next);
  ASVRL_SAC_ARRAY(eps_next);
  hipLaunchKernelGGL(sac_actor_fwd_kernel, dim3(sac_groups(io->B), 2), dim3(kSacT), 0, as_stream(stream),
                     SacActorFwdArgs{*local, *target, *io});
  return check_launch("asvrl_sac_actor_forward");
}

extern "C" int asvrl_sac_grad(const AsvDdpgWeights* local1, const AsvDdpgWeights* local2, const AsvDdpgWeights* target1,
                              const AsvDdpgWeights* target2, const AsvSacGradIO* io, void* stream) {
  const std::string who = "asvrl_sac_grad";
  if (int rc = ddpg_check_weights(who, "local1", local1, true)) return rc;
  if (int rc = ddpg_check_weights(who, "local2", local2, true)) return rc;
  if (int rc = ddpg_check_weights(who, "target1", target1, false)) return rc;
  if (int rc = ddpg_check_weights(who, "target2", target2, false)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
  ASVRL_SAC_ARRAY(logp_next);
  for (int k = 0; k < 2; ++k) {
    const AsvDdpgGradIO& c = io->c[k];
    const std::string pre = who + ": null array c" + std::to_string(k + 1) + ".";
#define ASVRL_SAC_C(name) ASVRL_REQUIRE(c.name != nullptr, pre + #name)
    ASVRL_SAC_C(rows);
    ASVRL_SAC_C(na);
    ASVRL_SAC_C(xb);
    ASVRL_SAC_C(h0);
    ASVRL_SAC_C(h1);
    ASVRL_SAC_C(p);
    ASVRL_SAC_C(h2);
    ASVRL_SAC_C(q);
    ASVRL_SAC_C(q_next);
    ASVRL_SAC_C(dq);
    ASVRL_SAC_C(dz2);
    ASVRL_SAC_C(dz1);
    ASVRL_SAC_C(dzG);
    ASVRL_SAC_C(dz0);
    ASVRL_SAC_C(tile_loss);
#undef ASVRL_SAC_C
    ASVRL_REQUIRE(reinterpret_cast<uintptr_t>(c.dzG) % 16 == 0, who + ": dzG must be 16-byte aligned");
    ASVRL_REQUIRE(c.ld_na >= 2, who + ": ld_na must be >= 2");
  }
  const AsvDdpgGradIO &c0 = io->c[0], &c1 = io->c[1];
  ASVRL_REQUIRE(c0.rows == c1.rows && c0.ld_rows == c1.ld_rows && c0.B == c1.B && c0.gamma == c1.gamma &&
                    c0.na == c1.na && c0.ld_na == c1.ld_na,
                who + ": c1 and c2 must share rows, ld_rows, B, gamma, na and ld_na");
  if (int rc = sac_check_rows(who, "rows", c0.rows, c0.ld_rows, c0.B, ASVRL_TR_DIM)) return rc;
  const int groups = sac_groups(c0.B);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(sac_fwd_kernel, dim3(groups, 4), dim3(kSacT), 0, st,
                     SacFwdArgs{{*local1, *local2, *target1, *target2}, *io});
  if (int rc = check_launch("asvrl_sac_grad(forward)")) return rc;
  hipLaunchKernelGGL(sac_bwd_kernel, dim3(groups, 2), dim3(kSacT), 0, st, SacBwdArgs{{*local1, *local2}, *io});
  return check_launch("asvrl_sac_grad(backward)");
}

extern "C" int asvrl_sac_actor_grad(const AsvDdpgWeights* local1, const AsvDdpgWeights* local2,
                                    const AsvSacActorGradIO* io, void* stream) {
  const std::string who = "asvrl_sac_actor_grad";
  if (int rc = ddpg_check_weights(who, "local1", local1, true)) return rc;
  if (int rc = ddpg_check_weights(who, "local2", local2, true)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
  ASVRL_SAC_ARRAY(act);
  ASVRL_SAC_ARRAY(q_pi);
  ASVRL_SAC_ARRAY(dA);
  if (int rc = sac_check_rows(who, "x", io->x, io->ldx, io->B, ASVRL_OBS_DIM)) return rc;
  ASVRL_REQUIRE(io->lda >= 2, who + ": lda must be >= 2");
  const dim3 grid(sac_groups(io->B), 2);
  hipStream_t st = as_stream(stream);
  const SacActorGradArgs args{{*local1, *local2}, *io};
  hipLaunchKernelGGL(sac_actor_q_kernel<false>, grid, dim3(kSacT), 0, st, args);
  if (int rc = check_launch("asvrl_sac_actor_grad(forward)")) return rc;
  hipLaunchKernelGGL(sac_actor_q_kernel<true>, grid, dim3(kSacT), 0, st, args);
  return check_launch("asvrl_sac_actor_grad(backward)");
}

extern "C" int asvrl_sac_actor_backward(const AsvSacActorWeights* w, const AsvSacActorIO* io, void* stream) {
  const std::string who = "asvrl_sac_actor_backward";
  if (int rc = sac_check_actor(who, "w", w, true)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
  ASVRL_REQUIRE(io->B >= 1 && io->B % 32 == 0, who + ": B must be a positive multiple of 32");
  ASVRL_SAC_ARRAY(h0);
  ASVRL_SAC_ARRAY(h1);
  ASVRL_SAC_ARRAY(h2);
  ASVRL_SAC_ARRAY(ls);
  ASVRL_SAC_ARRAY(sigma);
  ASVRL_SAC_ARRAY(z);
  ASVRL_SAC_ARRAY(a);
  ASVRL_SAC_ARRAY(eps);
  ASVRL_SAC_ARRAY(logp);
  ASVRL_SAC_ARRAY(dA);
  ASVRL_SAC_ARRAY(q_pi);
  ASVRL_SAC_ARRAY(dhead);
  ASVRL_SAC_ARRAY(dz2);
  ASVRL_SAC_ARRAY(dz1);
  ASVRL_SAC_ARRAY(dz0);
  ASVRL_SAC_ARRAY(tile_loss);
  hipLaunchKernelGGL(sac_actor_bwd_kernel, dim3(sac_groups(io->B)), dim3(kSacT), 0, as_stream(stream),
                     SacActorBwdArgs{*w, *io});
  return check_launch("asvrl_sac_actor_backward");
}

#undef ASVRL_SAC_ARRAY
