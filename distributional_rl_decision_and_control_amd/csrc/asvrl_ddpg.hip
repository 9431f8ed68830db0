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
  ddpg_bwd_tile(a.local, io, lane, rr, valid, a0, a1, dq);
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
  float d0, d1;
  ddpg_dA_tile(a.local, A, keep, lane, d0, d1);
  if (valid && h == 0) {
    io.dA[2 * rr] = d0;
    io.dA[2 * rr + 1] = d1;
  }
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
