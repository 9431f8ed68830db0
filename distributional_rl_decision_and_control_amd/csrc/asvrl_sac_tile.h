// asvrl_sac_tile.h -- SAC_model.Actor's head on the one-wave Actor tile (asvrl_actor_tile.h, trunk_chain): the f32
// head beside ActorLds, the Philox + Box-Muller noise of a row, and the reparameterised sample with its atan squash
// and log-probability (SAC_model.py:183-199).
// Shared by asvrl_sac.hip (sac_act_kernel, sac_actor_fwd_kernel) and asvrl_env.hip (env_policy_rollout_kernel<kPolSac>, the
// SAC act in front of every env step): the same dot products in the same order and the same Philox key, so a row's
// action does not depend on which kernel computed it.
#pragma once
#include "asvrl_actor_tile.h"

namespace asvrl {
namespace {
namespace sactile {
using namespace atile;

constexpr int kNHead = 2 * kNa;   // mu (2), log_std (2)
// Philox domain constants (counter word 3) of the three noise streams; explore()'s 0xAC7 and the env's are others
constexpr uint32_t kSacTargetStream = 0x5AC1u, kSacLocalStream = 0x5AC2u, kSacActStream = 0x5AC3u;
constexpr float kLogSqrt2Pi = 0.91893853320467274f;   // math.log(math.sqrt(2 * math.pi))
constexpr float kLsMin = -20.f, kLsMax = 2.f, kMinVal = 1e-6f;

// the head beside ActorLds: weight [4][128] (mu rows 0, 1; log_std rows 2, 3), then bias [4]
struct SacHeadLds {
  float w[kNHead * kHid], b[kNHead];
};
static_assert(sizeof(ActorLds) + sizeof(SacHeadLds) <= 160 * 1024, "the actor's images and the SAC head in one CU's LDS");

template <int T>
__device__ __forceinline__ void stage_head(SacHeadLds& H, const AsvSacActorWeights& w, int tid) {
  for (int i = tid; i < kNHead * kHid; i += T) H.w[i] = w.head[i];
  if (tid < kNHead) H.b[tid] = w.bhead[tid];
}

// two standard normals of (row, ctr) in noise stream `dom`: one Philox call, one Box-Muller pair
__device__ __forceinline__ void sac_eps(uint32_t dom, int row, uint64_t ctr, uint64_t seed, float& e0, float& e1) {
  const U4 u = philox4x32_10(U4{static_cast<uint32_t>(row), static_cast<uint32_t>(ctr),
                                static_cast<uint32_t>(ctr >> 32), dom},
                             static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  StreamF::box_muller_accurate(StreamF::u24(u.x), StreamF::u24(u.y), e0, e1);
}

struct SacSample {
  float mu[kNa], ls[kNa], sigma[kNa], z[kNa], a[kNa], logp;   // ls: before the clamp
};

// SAC_model.py:183-199 of the lane's row from h2 (trunk_chain's groups) and its eps. Every lane of the wave must be
// live (one exchange between the lane halves); both lanes of the row's pair end with the same values.
// LOGP false (the act inside the env's step loop, which needs the action only): o.logp is left unwritten.
template <bool LOGP = true>
__device__ __forceinline__ void sac_head(const SacHeadLds& H, float scale, const float (&h2v)[8][8], int lane,
                                         const float (&eps)[kNa], SacSample& o) {
  const int h = lane >> 5;
  float p[kNHead] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = feat(mb, 8 * s + j, h);
        const float v = h2v[mb * 2 + s][j];
#pragma unroll
        for (int k = 0; k < kNHead; ++k) p[k] += H.w[k * kHid + m] * v;
      }
#pragma unroll
  for (int k = 0; k < kNHead; ++k) p[k] = p[k] + __shfl_xor(p[k], 32, 64) + H.b[k];
  if constexpr (LOGP) o.logp = 0.f;
#pragma unroll
  for (int d = 0; d < kNa; ++d) {
    o.mu[d] = p[d];
    o.ls[d] = p[kNa + d];
    const float ls = fminf(fmaxf(o.ls[d], kLsMin), kLsMax);
    o.sigma[d] = expf(ls);
    o.z[d] = o.mu[d] + o.sigma[d] * eps[d];   // Normal.rsample
    o.a[d] = scale * atanf(o.z[d]);
    // Normal.log_prob(z) with (z - mu) / sigma = eps, minus the squash's log-derivative term
    if constexpr (LOGP)
      o.logp += ((-(eps[d] * eps[d]) * 0.5f - ls) - kLogSqrt2Pi) - logf((1.f - o.a[d] * o.a[d]) + kMinVal);
  }
}

}  // namespace sactile
}  // namespace
}  // namespace asvrl
