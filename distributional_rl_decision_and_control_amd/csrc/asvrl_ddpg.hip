// asvrl_ddpg.hip -- DDPG's critic (agent.py:478-516 train_DDPG) on MFMA (gfx950). DDPG_model.Critic is the
// AC-IQN critic without the cosine embedding and with one scalar per sample: both observation encoders as one
// block-structured 256 x 32 matrix -> F, hidden_layer 256 -> 128 (h1), the product with G = relu(Wae a + bae),
// hidden_layer_2 128 -> 128 (h2) and a 128 -> 1 output. That is row-per-sample work, so every kernel here runs
// the one-wave Actor tile of asvrl_actor_tile.h (the chain itself: ddpg_q_tile, asvrl_ddpg_tile.h) the way
// asvrl_dqn.hip does. DDPG's Actor is the AC-IQN Actor and runs asvrl_mlp.hip's kernels as they are.
//
// Kernels:
//   ddpg_fwd_kernel    the critic update's two forwards in one launch: blockIdx.y = 0 the local critic on (s, a)
//                      of the replay rows saving the activations and q; blockIdx.y = 1 the target critic on
//                      (s', na) -> q_next, na the target actor's action (asvrl_actor_forward beforehand)
//   ddpg_bwd_kernel    y = r + gamma (1 - d) q_next, smooth-L1 (beta 1) per-tile loss partials, dq, and the
//                      backward to every layer's pre-activation gradient (dz2, dz1, dzG, dzF); no LDS, no barrier
//   ddpg_actor_kernel  the actor step through the updated critic: forward Q(s, a_pi), backward of -mean q as far
//                      as dzG, dA = Wae^T dzG, per-tile partials of the actor loss; no saved activations
// The weight gradients are the project's batched reduction over (dz, saved activation) pairs
// (asvrl_linear_wgrad_multi + asvrl_partial_sums_norm, fused_ddpg.py).
#include "asvrl_common.h"
#include "asvrl_mfma.h"
#include "asvrl_lds.h"
#include "asvrl_actor_tile.h"
#include "asvrl_ddpg_tile.h"

namespace asvrl {
namespace {
using namespace atile;
using namespace ddtile;

constexpr int kDdpgWaves = 4;
constexpr int kActCol = 2 * ASVRL_OBS_DIM;   // replay row: action (2), reward, done behind s and s'

struct DdpgFwdArgs {
  AsvDdpgWeights local, target;
  AsvDdpgGradIO io;
};

__global__ __launch_bounds__(kDdpgWaves * 64) void ddpg_fwd_kernel(DdpgFwdArgs a) {
  __shared__ ActorLds L;
  __shared__ AeLds A;
  const AsvDdpgGradIO& io = a.io;
  const bool tgt = blockIdx.y != 0;   // workgroup-uniform
  const AsvDdpgWeights& w = tgt ? a.target : a.local;
  const int tile = blockIdx.x * kDdpgWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
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
  stage_actor<kDdpgWaves * 64>(L, w.trunk, threadIdx.x);
  stage_ae<kDdpgWaves * 64>(A, w, threadIdx.x);
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

// 16 saved activations of block mb of the lane's row in accumulator order (register g <-> feat(mb, g, h))
__device__ __forceinline__ void ddpg_load16(const elem_t* rowp, int mb, int h, float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 16; g += 4) load4(rowp + mb * 32 + 8 * (g >> 2) + 4 * h, &v[g]);
}

struct DdpgBwdArgs {
  AsvDdpgWeights local;
  AsvDdpgGradIO io;
};

__global__ __launch_bounds__(kDdpgWaves * 64) void ddpg_bwd_kernel(DdpgBwdArgs a) {
  const AsvDdpgGradIO& io = a.io;
  const int tile = blockIdx.x * kDdpgWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile * 32 >= io.B) return;   // whole waves; the kernel has no barrier
  const int h = lane >> 5, r = lane & 31;
  const int row = tile * 32 + r;
  const bool valid = row < io.B;
  const int64_t rr = valid ? row : io.B - 1;
  // ---------------- target, loss and dq (agent.py:488-497)
  const float* rp = io.rows + rr * io.ld_rows + kActCol;
  const float a0 = rp[0], a1 = rp[1], rew = rp[2], done = rp[3];
  const float y = rew + io.gamma * io.q_next[rr] * (1.f - done);
  const float diff = io.q[rr] - y;
  const float ad = fabsf(diff);
  const float inv_b = 1.f / static_cast<float>(io.B);
  float lossv = (valid && h == 0) ? (ad < 1.f ? 0.5f * diff * diff : ad - 0.5f) * inv_b : 0.f;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossv += __shfl_xor(lossv, off, 64);
  if (lane == 0) io.tile_loss[tile] = lossv;
  const float dq = valid ? fminf(fmaxf(diff, -1.f), 1.f) * inv_b : 0.f;
  if (valid && h == 0) io.dq[row] = dq;
  // ---------------- dz2 = dq wo 1[z2 > 0]
  const float* wo = a.local.trunk.wout;
  frag8 dz2pk[8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    float hv[16];
    ddpg_load16(bp(io.h2) + rr * kHid, mb, h, hv);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dv[j] = hv[8 * s + j] > 0.f ? wo[feat(mb, 8 * s + j, h)] * dq : 0.f;
      dz2pk[mb * 2 + s] = pack8(dv);
      store16(valid ? bp(io.dz2) + rr * kHid + mb * 32 + 16 * s : nullptr, dv, h);
    }
  }
  // ---------------- dp = W2^T dz2; dz1 = dp G 1[z1 > 0], dzG = dp h1 1[G > 0]
  const frag8* W2T = reinterpret_cast<const frag8*>(a.local.trunk.w2t_frag);
  const frag8* W1T = reinterpret_cast<const frag8*>(a.local.trunk.w1t_frag);
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
      float dv[8], dg[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = ae_feature(a.local.wae, a.local.bae, feat(mb, 8 * s + j, h), a0, a1);
        const float hj = hv[8 * s + j], dp = acc[8 * s + j];
        dv[j] = hj > 0.f ? dp * g : 0.f;
        dg[j] = g > 0.f ? dp * hj : 0.f;
      }
      dz1pk[mb * 2 + s] = pack8(dv);
      store16(valid ? bp(io.dz1) + rr * kHid + mb * 32 + 16 * s : nullptr, dv, h);
      if (valid) {   // f32: the lane's two 4-feature pieces of the group
        float* gp = io.dzG + rr * kHid + mb * 32 + 16 * s + 4 * h;
        *reinterpret_cast<f32x4*>(gp) = f32x4{dg[0], dg[1], dg[2], dg[3]};
        *reinterpret_cast<f32x4*>(gp + 8) = f32x4{dg[4], dg[5], dg[6], dg[7]};
      }
    }
  }
  // ---------------- dzF = (W1^T dz1) 1[F > 0] (a masked object's F is 0: no gradient reaches it)
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

struct DdpgActorArgs {
  AsvDdpgWeights local;
  AsvDdpgActorIO io;
};

__global__ __launch_bounds__(kDdpgWaves * 64) void ddpg_actor_kernel(DdpgActorArgs a) {
  __shared__ ActorLds L;
  __shared__ AeLds A;
  const AsvDdpgActorIO& io = a.io;
  const int tile = blockIdx.x * kDdpgWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
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
  stage_actor<kDdpgWaves * 64>(L, a.local.trunk, threadIdx.x);
  stage_ae<kDdpgWaves * 64>(A, a.local, threadIdx.x);
  __syncthreads();   // the only barrier: before any wave leaves
  if (!active) return;
  const int h = lane >> 5;
  // loss = -mean q: dq = -1 / B on every row
  const float dq = -1.f / static_cast<float>(io.B);
  ActorKeep keep;
  const float q = ddpg_q_tile<DD_ACTOR>(a.local.trunk, AsvDdpgGradIO{}, L, A, row, valid, lane, bx, mk, a0, a1, dq, &keep);
  float lossv = (valid && h == 0) ? q * dq : 0.f;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossv += __shfl_xor(lossv, off, 64);
  if (lane == 0) io.tile_loss[tile] = lossv;
  if (valid && h == 0 && io.q != nullptr) io.q[row] = q;
  // dp = W2^T dz2; dzG = dp h1 1[G > 0]; dA = Wae^T dzG
  const frag8* W2T = reinterpret_cast<const frag8*>(a.local.trunk.w2t_frag);
  float d0 = 0.f, d1 = 0.f;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    f32x16 acc = f32x16{};
#pragma unroll
    for (int ks = 0; ks < kHid / 16; ++ks) acc = mfma(W2T[(mb * 8 + ks) * 64 + lane], keep.dz2pk[ks], acc);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int m = feat(mb, g, h);
      const float dg = acc[g] * keep.t[mb][g];
      d0 += A.w[2 * m] * dg;
      d1 += A.w[2 * m + 1] * dg;
    }
  }
  d0 += __shfl_xor(d0, 32, 64);   // every lane of the wave is live here
  d1 += __shfl_xor(d1, 32, 64);
  if (valid && h == 0) {
    io.dA[2 * rr] = d0;
    io.dA[2 * rr + 1] = d1;
  }
}

int ddpg_check_weights(const std::string& who, const char* name, const AsvDdpgWeights* w, bool backward) {
  ASVRL_REQUIRE(w != nullptr, who + ": null struct " + name);
  const std::string pre = who + ": null array " + name + ".";
#define ASVRL_DDPG_W(field, ptr) ASVRL_REQUIRE((ptr) != nullptr, pre + field)
  ASVRL_DDPG_W("enc_frag", w->trunk.enc_frag);
  ASVRL_DDPG_W("b_enc", w->trunk.b_enc);
  ASVRL_DDPG_W("w1_frag", w->trunk.w1_frag);
  ASVRL_DDPG_W("w2_frag", w->trunk.w2_frag);
  ASVRL_DDPG_W("b1", w->trunk.b1);
  ASVRL_DDPG_W("b2", w->trunk.b2);
  ASVRL_DDPG_W("wout", w->trunk.wout);
  ASVRL_DDPG_W("bout", w->trunk.bout);
  ASVRL_DDPG_W("wae", w->wae);
  ASVRL_DDPG_W("bae", w->bae);
  if (backward) {
    ASVRL_DDPG_W("w2t_frag", w->trunk.w2t_frag);
    ASVRL_DDPG_W("w1t_frag", w->trunk.w1t_frag);
  }
#undef ASVRL_DDPG_W
  return 0;
}

}  // namespace
}  // namespace asvrl

using namespace asvrl;

extern "C" int64_t asvrl_ddpg_weights_struct_size(void) { return sizeof(AsvDdpgWeights); }
extern "C" int64_t asvrl_ddpg_grad_struct_size(void) { return sizeof(AsvDdpgGradIO); }
extern "C" int64_t asvrl_ddpg_actor_struct_size(void) { return sizeof(AsvDdpgActorIO); }

extern "C" int asvrl_ddpg_grad(const AsvDdpgWeights* local, const AsvDdpgWeights* target, const AsvDdpgGradIO* io,
                               void* stream) {
  const std::string who = "asvrl_ddpg_grad";
  if (int rc = ddpg_check_weights(who, "local", local, true)) return rc;
  if (int rc = ddpg_check_weights(who, "target", target, false)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
#define ASVRL_DDPG_ARRAY(name) ASVRL_REQUIRE(io->name != nullptr, who + ": null array " #name)
  ASVRL_DDPG_ARRAY(rows);
  ASVRL_DDPG_ARRAY(na);
  ASVRL_DDPG_ARRAY(xb);
  ASVRL_DDPG_ARRAY(h0);
  ASVRL_DDPG_ARRAY(h1);
  ASVRL_DDPG_ARRAY(p);
  ASVRL_DDPG_ARRAY(h2);
  ASVRL_DDPG_ARRAY(q);
  ASVRL_DDPG_ARRAY(q_next);
  ASVRL_DDPG_ARRAY(dq);
  ASVRL_DDPG_ARRAY(dz2);
  ASVRL_DDPG_ARRAY(dz1);
  ASVRL_DDPG_ARRAY(dzG);
  ASVRL_DDPG_ARRAY(dz0);
  ASVRL_DDPG_ARRAY(tile_loss);
#undef ASVRL_DDPG_ARRAY
  ASVRL_REQUIRE(io->B >= 1 && io->B % 32 == 0, who + ": B must be a positive multiple of 32");
  ASVRL_REQUIRE(io->ld_rows >= ASVRL_TR_DIM && io->ld_rows % 4 == 0 && reinterpret_cast<uintptr_t>(io->rows) % 16 == 0,
                who + ": rows must be 16-byte aligned replay rows");
  ASVRL_REQUIRE(io->ld_na >= 2, who + ": ld_na must be >= 2");
  ASVRL_REQUIRE(reinterpret_cast<uintptr_t>(io->dzG) % 16 == 0, who + ": dzG must be 16-byte aligned");
  const int tiles = io->B / 32, groups = (tiles + kDdpgWaves - 1) / kDdpgWaves;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ddpg_fwd_kernel, dim3(groups, 2), dim3(kDdpgWaves * 64), 0, st, DdpgFwdArgs{*local, *target, *io});
  if (int rc = check_launch("asvrl_ddpg_grad(forward)")) return rc;
  hipLaunchKernelGGL(ddpg_bwd_kernel, dim3(groups), dim3(kDdpgWaves * 64), 0, st, DdpgBwdArgs{*local, *io});
  return check_launch("asvrl_ddpg_grad(backward)");
}

extern "C" int asvrl_ddpg_actor_grad(const AsvDdpgWeights* local, const AsvDdpgActorIO* io, void* stream) {
  const std::string who = "asvrl_ddpg_actor_grad";
  if (int rc = ddpg_check_weights(who, "local", local, true)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
  ASVRL_REQUIRE(io->x != nullptr, who + ": null array x");
  ASVRL_REQUIRE(io->act != nullptr, who + ": null array act");
  ASVRL_REQUIRE(io->dA != nullptr, who + ": null array dA");
  ASVRL_REQUIRE(io->tile_loss != nullptr, who + ": null array tile_loss");
  ASVRL_REQUIRE(io->B >= 1 && io->B % 32 == 0, who + ": B must be a positive multiple of 32");
  ASVRL_REQUIRE(io->ldx >= ASVRL_OBS_DIM && io->ldx % 4 == 0 && reinterpret_cast<uintptr_t>(io->x) % 16 == 0,
                who + ": x rows must be 16-byte aligned");
  ASVRL_REQUIRE(io->lda >= 2, who + ": lda must be >= 2");
  const int tiles = io->B / 32, groups = (tiles + kDdpgWaves - 1) / kDdpgWaves;
  hipLaunchKernelGGL(ddpg_actor_kernel, dim3(groups), dim3(kDdpgWaves * 64), 0, as_stream(stream),
                     DdpgActorArgs{*local, *io});
  return check_launch("asvrl_ddpg_actor_grad");
}
