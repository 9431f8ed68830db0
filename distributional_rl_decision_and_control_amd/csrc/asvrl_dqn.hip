// asvrl_dqn.hip -- DQN (agent.py:271-287 act_dqn, :518-545 train_DQN) on MFMA (gfx950). DQN_Policy
// (DQN_model.py) is the AC-IQN Actor's trunk layer for layer -- both observation encoders as one
// block-structured 256 x 32 matrix, hidden_layer 256 -> 128, hidden_layer_2 128 -> 128 -- with a 128 -> A
// output layer (A = 25) and no squash, so every kernel here runs the one-wave Actor tile of
// asvrl_actor_tile.h (trunk_chain) and adds the head: the output layer padded to 32 rows as one chained
// 32 x 128 fragment image (rows A.. zero), eight MFMAs per 32-row tile. Accumulator register g of lane half
// h then holds Q[feat(0, g, h)] of the lane's row; columns >= A are never read (max, arg-max, gather) and
// never written (dz_out keeps them zero).
//
// Kernels:
//   dqn_act_kernel   Q on every robot row, arg-max (first maximum, np.argmax), epsilon-greedy on the device
//                    step counter (the keyed Philox draw of the IQN act kernel), f64 action index; optional Q rows
//   dqn_fwd_kernel   the update's two forwards in one launch: blockIdx.y = 0 the local net on s saving the
//                    activations and q = Q(s)[a]; blockIdx.y = 1 the target net on s' -> q_next = max_a Q
//   dqn_bwd_kernel   y = r + (1 - d) gamma q_next, smooth-L1 (beta 1) per-tile loss partials, dQ, and the
//                    backward to every layer's pre-activation gradient (dz_out, dz2, dz1, dz0); no LDS, no barrier
//   dqn_head_pack_kernel  the head image from output_layer.weight
// The weight gradients are the project's batched reduction over (dz, saved activation) pairs
// (asvrl_linear_wgrad_multi + asvrl_partial_sums_norm, fused_dqn.py).
#include "asvrl_common.h"
#include "asvrl_mfma.h"
#include "asvrl_lds.h"
#include "asvrl_actor_tile.h"
#include "asvrl_dqn_tile.h"

namespace asvrl {
namespace {
using namespace atile;
using namespace dqtile;

constexpr int kDqnWaves = 4;

struct DqnActArgs {
  AsvDqnWeights w;
  AsvDqnActIO io;
};

__global__ __launch_bounds__(kDqnWaves * 64) void dqn_act_kernel(DqnActArgs a) {
  __shared__ ActorLds L;
  const AsvDqnActIO& io = a.io;
  const int tile = blockIdx.x * kDqnWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool active = tile * 32 < io.n;
  frag8 bx[2];
  float mk[kObjN];
  const int row = tile * 32 + (lane & 31);
  const bool valid = active && row < io.n;
  if (active) load_obs(io.x, io.ldx, valid ? row : io.n - 1, lane >> 5, bx, mk);
  stage_actor<kDqnWaves * 64>(L, a.w.trunk, threadIdx.x);
  __syncthreads();   // the only barrier: before any wave leaves
  if (!active) return;
  const int h = lane >> 5, A = a.w.n_actions;
  float q[16];
  dqn_q_tile<MLP_ACT>(a.w, AsvMlpIO{}, L, row, valid, lane, bx, mk, q);
  float best;
  int bi;
  dqn_argmax(q, h, A, best, bi);
  if (!valid) return;
  if (io.q_out != nullptr) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int m = feat(0, g, h);
      if (m < A) io.q_out[static_cast<int64_t>(row) * A + m] = q[g];
    }
  }
  if (h != 0) return;
  // epsilon-greedy on the device step counter: dqn_explore (asvrl_dqn_tile.h), shared with the closed-loop windows
  const uint64_t step = io.step_dev != nullptr ? static_cast<uint64_t>(*io.step_dev) : 0ull;
  const int act = dqn_explore(step, EpsSchedule{io.eps_steps_per_count, io.eps_total, io.eps_fraction, io.eps_initial,
                                                io.eps_final},
                              io.seed, row, bi, A);
  double* o = io.act_out + static_cast<int64_t>(row) * io.ld_act;
  o[0] = static_cast<double>(act);
  o[1] = 0.0;
}

struct DqnFwdArgs {
  AsvDqnWeights local, target;
  AsvMlpIO save;   // xb, h0, h1, h2 of the local pass
  AsvDqnGradIO io;
};

// the taken action of replay row b (column 80, a float index), -1 when outside the head
__device__ __forceinline__ int dqn_action(const AsvDqnGradIO& io, int b, int A) {
  const int a = static_cast<int>(io.rows[static_cast<int64_t>(b) * io.ld_rows + 2 * ASVRL_OBS_DIM]);
  return (a >= 0 && a < A) ? a : -1;
}

__global__ __launch_bounds__(kDqnWaves * 64) void dqn_fwd_kernel(DqnFwdArgs a) {
  __shared__ ActorLds L;
  const AsvDqnGradIO& io = a.io;
  const bool tgt = blockIdx.y != 0;   // workgroup-uniform
  const AsvDqnWeights& w = tgt ? a.target : a.local;
  const int tile = blockIdx.x * kDqnWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool active = tile * 32 < io.B;
  const float* x = io.rows + (tgt ? ASVRL_OBS_DIM : 0);
  frag8 bx[2];
  float mk[kObjN];
  const int row = tile * 32 + (lane & 31);
  const bool valid = active && row < io.B;
  if (active) load_obs(x, io.ld_rows, valid ? row : io.B - 1, lane >> 5, bx, mk);
  stage_actor<kDqnWaves * 64>(L, w.trunk, threadIdx.x);
  __syncthreads();   // the only barrier: before any wave leaves
  if (!active) return;
  const int h = lane >> 5, A = w.n_actions;
  float q[16];
  if (tgt) {
    dqn_q_tile<MLP_FWD>(w, a.save, L, row, valid, lane, bx, mk, q);
    float best;
    int bi;
    dqn_argmax(q, h, A, best, bi);
    if (valid && h == 0) io.q_next[row] = best;
  } else {
    dqn_q_tile<MLP_TRAIN>(w, a.save, L, row, valid, lane, bx, mk, q);
    const int act = dqn_action(io, valid ? row : io.B - 1, A);
    float sel = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) sel += feat(0, g, h) == act ? q[g] : 0.f;
    sel += __shfl_xor(sel, 32, 64);   // the other half holds 0 (or the value): exact
    if (valid && h == 0) io.q_sel[row] = sel;
  }
}

// 16 saved activations of block mb of the lane's row in accumulator order (register g <-> feat(mb, g, h))
__device__ __forceinline__ void dqn_load16(const elem_t* rowp, int mb, int h, float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 16; g += 4) load4(rowp + mb * 32 + 8 * (g >> 2) + 4 * h, &v[g]);
}

struct DqnBwdArgs {
  AsvDqnWeights local;
  AsvDqnGradIO io;
};

__global__ __launch_bounds__(kDqnWaves * 64) void dqn_bwd_kernel(DqnBwdArgs a) {
  const AsvDqnGradIO& io = a.io;
  const int tile = blockIdx.x * kDqnWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (tile * 32 >= io.B) return;   // whole waves; the kernel has no barrier
  const int h = lane >> 5, r = lane & 31, A = a.local.n_actions;
  const int row = tile * 32 + r;
  const bool valid = row < io.B;
  const int64_t rr = valid ? row : io.B - 1;
  // ---------------- target, loss and dQ (agent.py:531-538)
  const float* rp = io.rows + rr * io.ld_rows + 2 * ASVRL_OBS_DIM;
  const int act = dqn_action(io, static_cast<int>(rr), A);
  const float rew = rp[2], done = rp[3];
  const float t = (1.f - done) * io.gamma;
  const float y = rew + t * io.q_next[rr];
  const float diff = io.q_sel[rr] - y;
  const float ad = fabsf(diff);
  const float inv_b = 1.f / static_cast<float>(io.B);
  float lossv = (valid && h == 0 && act >= 0) ? (ad < 1.f ? 0.5f * diff * diff : ad - 0.5f) * inv_b : 0.f;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossv += __shfl_xor(lossv, off, 64);
  if (lane == 0) io.tile_loss[tile] = lossv;
  const float dq = (valid && act >= 0) ? fminf(fmaxf(diff, -1.f), 1.f) * inv_b : 0.f;
  // ---------------- dz_out: dQ at the taken action, zero elsewhere (the padded columns included)
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = feat(0, 8 * s + j, h) == act ? dq : 0.f;
    store16(valid ? bp(io.dz_out) + rr * kQPad + 16 * s : nullptr, v, h);
  }
  // ---------------- dz2 = Wout[a]^T dQ 1[h2 > 0]
  const float* wo = a.local.trunk.wout + static_cast<int64_t>(act >= 0 ? act : 0) * kHid;
  frag8 dz2pk[8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    float hv[16];
    dqn_load16(bp(io.h2) + rr * kHid, mb, h, hv);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dv[j] = hv[8 * s + j] > 0.f ? wo[feat(mb, 8 * s + j, h)] * dq : 0.f;
      dz2pk[mb * 2 + s] = pack8(dv);
      store16(valid ? bp(io.dz2) + rr * kHid + mb * 32 + 16 * s : nullptr, dv, h);
    }
  }
  // ---------------- dz1 = (W2^T dz2) 1[h1 > 0]
  const frag8* W2T = reinterpret_cast<const frag8*>(a.local.trunk.w2t_frag);
  const frag8* W1T = reinterpret_cast<const frag8*>(a.local.trunk.w1t_frag);
  frag8 dz1pk[8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    float hv[16];
    dqn_load16(bp(io.h1) + rr * kHid, mb, h, hv);
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
  // ---------------- dz0 = (W1^T dz1) 1[h0 > 0] (a masked object's h0 is 0: no gradient reaches it)
#pragma unroll
  for (int mb = 0; mb < 8; ++mb) {
    float hv[16];
    dqn_load16(bp(io.h0) + rr * kEnc, mb, h, hv);
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

__global__ __launch_bounds__(256) void dqn_head_pack_kernel(const float* __restrict__ wout, int A, elem_t* img) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= kQPad * kHid) return;
  int row, col;
  frag_rc(o, kHid, true, row, col);
  img[o] = (elem_t)(row < A ? wout[row * kHid + col] : 0.f);
}

int dqn_check_weights(const std::string& who, const char* name, const AsvDqnWeights* w, bool backward) {
  ASVRL_REQUIRE(w != nullptr, who + ": null struct " + name);
  const std::string pre = who + ": null array " + name + ".";
#define ASVRL_DQN_W(field, ptr) ASVRL_REQUIRE((ptr) != nullptr, pre + field)
  ASVRL_DQN_W("enc_frag", w->trunk.enc_frag);
  ASVRL_DQN_W("b_enc", w->trunk.b_enc);
  ASVRL_DQN_W("w1_frag", w->trunk.w1_frag);
  ASVRL_DQN_W("w2_frag", w->trunk.w2_frag);
  ASVRL_DQN_W("b1", w->trunk.b1);
  ASVRL_DQN_W("b2", w->trunk.b2);
  ASVRL_DQN_W("wout", w->trunk.wout);
  ASVRL_DQN_W("bout", w->trunk.bout);
  ASVRL_DQN_W("head_frag", w->head_frag);
  if (backward) {
    ASVRL_DQN_W("w2t_frag", w->trunk.w2t_frag);
    ASVRL_DQN_W("w1t_frag", w->trunk.w1t_frag);
  }
#undef ASVRL_DQN_W
  // >= 2: the tile's staging reads the first two output rows (the Actor's whole output layer)
  ASVRL_REQUIRE(w->n_actions >= 2 && w->n_actions <= kQPad, who + ": " + name + ".n_actions must be in 2..32");
  return 0;
}

}  // namespace
}  // namespace asvrl

using namespace asvrl;

extern "C" int64_t asvrl_dqn_weights_struct_size(void) { return sizeof(AsvDqnWeights); }
extern "C" int64_t asvrl_dqn_act_struct_size(void) { return sizeof(AsvDqnActIO); }
extern "C" int64_t asvrl_dqn_grad_struct_size(void) { return sizeof(AsvDqnGradIO); }

extern "C" int asvrl_dqn_pack(const AsvMlpSrc* src, const float* wout, const AsvDqnWeights* w, void* stream) {
  const std::string who = "asvrl_dqn_pack";
  ASVRL_REQUIRE(src != nullptr, who + ": null struct src");
  ASVRL_REQUIRE(wout != nullptr, who + ": null array wout");
  ASVRL_REQUIRE(src->w1 != nullptr, who + ": null array src.w1");
  if (int rc = dqn_check_weights(who, "w", w, true)) return rc;
  if (int rc = asvrl_mlp_pack(src, &w->trunk, stream)) return rc;
  hipLaunchKernelGGL(dqn_head_pack_kernel, dim3(kQPad * kHid / 256), dim3(256), 0, as_stream(stream), wout,
                     w->n_actions, const_cast<elem_t*>(static_cast<const elem_t*>(w->head_frag)));
  return check_launch("asvrl_dqn_pack");
}

extern "C" int asvrl_dqn_act(const AsvDqnWeights* w, const AsvDqnActIO* io, void* stream) {
  const std::string who = "asvrl_dqn_act";
  if (int rc = dqn_check_weights(who, "w", w, false)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
  ASVRL_REQUIRE(io->x != nullptr, who + ": null array x");
  ASVRL_REQUIRE(io->act_out != nullptr, who + ": null array act_out");
  ASVRL_REQUIRE(io->n >= 0, who + ": n must be >= 0");
  ASVRL_REQUIRE(io->ld_act >= 2, who + ": ld_act must be >= 2");
  ASVRL_REQUIRE(io->eps_total > 0.0 && io->eps_fraction > 0.0, who + ": eps_total and eps_fraction must be > 0");
  ASVRL_REQUIRE(io->ldx % 4 == 0 && reinterpret_cast<uintptr_t>(io->x) % 16 == 0,
                who + ": x rows must be 16-byte aligned");
  if (io->n == 0) return 0;
  const int tiles = (io->n + 31) / 32;
  hipLaunchKernelGGL(dqn_act_kernel, dim3((tiles + kDqnWaves - 1) / kDqnWaves), dim3(kDqnWaves * 64), 0,
                     as_stream(stream), DqnActArgs{*w, *io});
  return check_launch("asvrl_dqn_act");
}

extern "C" int asvrl_dqn_grad(const AsvDqnWeights* local, const AsvDqnWeights* target, const AsvDqnGradIO* io,
                              void* stream) {
  const std::string who = "asvrl_dqn_grad";
  if (int rc = dqn_check_weights(who, "local", local, true)) return rc;
  if (int rc = dqn_check_weights(who, "target", target, false)) return rc;
  ASVRL_REQUIRE(io != nullptr, who + ": null struct io");
#define ASVRL_DQN_ARRAY(name) ASVRL_REQUIRE(io->name != nullptr, who + ": null array " #name)
  ASVRL_DQN_ARRAY(rows);
  ASVRL_DQN_ARRAY(xb);
  ASVRL_DQN_ARRAY(h0);
  ASVRL_DQN_ARRAY(h1);
  ASVRL_DQN_ARRAY(h2);
  ASVRL_DQN_ARRAY(q_sel);
  ASVRL_DQN_ARRAY(q_next);
  ASVRL_DQN_ARRAY(dz_out);
  ASVRL_DQN_ARRAY(dz2);
  ASVRL_DQN_ARRAY(dz1);
  ASVRL_DQN_ARRAY(dz0);
  ASVRL_DQN_ARRAY(tile_loss);
#undef ASVRL_DQN_ARRAY
  ASVRL_REQUIRE(io->B >= 1 && io->B % 32 == 0, who + ": B must be a positive multiple of 32");
  ASVRL_REQUIRE(local->n_actions == target->n_actions, who + ": local and target n_actions differ");
  ASVRL_REQUIRE(io->ld_rows >= ASVRL_TR_DIM && io->ld_rows % 4 == 0 && reinterpret_cast<uintptr_t>(io->rows) % 16 == 0,
                who + ": rows must be 16-byte aligned replay rows");
  AsvMlpIO save{};
  save.n = io->B;
  save.xb = io->xb;
  save.h0 = io->h0;
  save.h1 = io->h1;
  save.h2 = io->h2;
  const int tiles = io->B / 32, groups = (tiles + kDqnWaves - 1) / kDqnWaves;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(dqn_fwd_kernel, dim3(groups, 2), dim3(kDqnWaves * 64), 0, st, DqnFwdArgs{*local, *target, save, *io});
  if (int rc = check_launch("asvrl_dqn_grad(forward)")) return rc;
  hipLaunchKernelGGL(dqn_bwd_kernel, dim3(groups), dim3(kDqnWaves * 64), 0, st, DqnBwdArgs{*local, *io});
  return check_launch("asvrl_dqn_grad(backward)");
}
