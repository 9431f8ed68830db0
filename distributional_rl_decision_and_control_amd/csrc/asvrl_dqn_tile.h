// asvrl_dqn_tile.h -- DQN_Policy's head on the one-wave Actor tile (asvrl_actor_tile.h, trunk_chain): the Q values
// of a 32-row tile, their first arg-max, and the epsilon-greedy choice of the batched act (agent.py:271-287).
// Shared by asvrl_dqn.hip (dqn_act_kernel, dqn_fwd_kernel) and asvrl_env.hip (env_policy_rollout_kernel<kPolDqn>, the DQN
// act in front of every env step): the same MFMAs in the same order and the same Philox key, so a row's action does
// not depend on which kernel computed it.
#pragma once
#include "asvrl_actor_tile.h"

namespace asvrl {
namespace {
namespace dqtile {
using namespace atile;

constexpr int kQPad = ASVRL_DQN_MAX_ACTIONS;   // head rows in the image (one 32-feature block)
static_assert(kQPad == 32, "the head is one MFMA feature block");

// Q of the lane's row: registers g <-> action feat(0, g, h). MODE MLP_TRAIN saves xb / h0 / h1 / h2.
template <int MODE>
__device__ __forceinline__ void dqn_q_tile(const AsvDqnWeights& w, const AsvMlpIO& io, const ActorLds& L, int row,
                                           bool valid, int lane, const frag8 (&bx)[2], const float (&mk)[kObjN],
                                           float (&q)[16]) {
  const int h = lane >> 5;
  if (MODE == MLP_TRAIN && valid) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      *reinterpret_cast<frag8*>(bp(io.xb) + static_cast<int64_t>(row) * kObsK + ks * 16 + 8 * h) = bx[ks];
  }
  float h2v[8][8];
  trunk_chain<MODE>(w.trunk, io, L, row, valid, lane, bx, mk, h2v);
  const frag8* HW = reinterpret_cast<const frag8*>(w.head_frag);
  f32x16 acc = f32x16{};
#pragma unroll
  for (int ks = 0; ks < kHid / 16; ++ks) acc = mfma(HW[ks * 64 + lane], pack8(h2v[ks]), acc);
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int m = feat(0, g, h);
    q[g] = acc[g] + (m < w.n_actions ? w.trunk.bout[m] : 0.f);
  }
}

// max and first arg-max over the A real outputs of the row (both lane halves end with the row's result)
__device__ __forceinline__ void dqn_argmax(const float (&q)[16], int h, int A, float& best, int& bi) {
  best = -__builtin_inff();
  bi = kQPad;
#pragma unroll
  for (int g = 0; g < 16; ++g) {   // feat(0, g, h) increases with g: the first maximum of the half
    const int m = feat(0, g, h);
    if (m < A && q[g] > best) {
      best = q[g];
      bi = m;
    }
  }
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bi, 32, 64);
  if (ob > best || (ob == best && oi < bi)) {
    best = ob;
    bi = oi;
  }
}

// epsilon-greedy (agent.py:271-287): the linear schedule of the step count (trainer.py:257-264); greedy (the
// arg-max bi) iff random() > eps, else random.choice(np.arange(action_size)). The draw is keyed by (row, step) and
// the policy's seed -- the IQN act kernel's draw. Returns the action index.
__device__ __forceinline__ int dqn_explore(uint64_t step, const EpsSchedule& s, uint64_t seed, int row, int bi, int A) {
  const double progress = static_cast<double>(step) * s.steps_per_count / s.total;
  const double eps = progress < s.fraction ? s.eps_initial + (progress / s.fraction) * (s.eps_final - s.eps_initial)
                                            : s.eps_final;
  const U4 u = philox4x32_10(U4{static_cast<uint32_t>(row), static_cast<uint32_t>(step),
                                static_cast<uint32_t>(step >> 32), 0x1A8u},
                             static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  const double c = (static_cast<double>(u.x >> 8) + 1.0) * (1.0 / 16777216.0);   // random() in (0, 1]
  int act = bi < A ? bi : 0;
  if (!(c > eps)) act = static_cast<int>((static_cast<uint64_t>(u.y >> 8) * static_cast<uint64_t>(A)) >> 24);
  return act;
}

}  // namespace dqtile
}  // namespace
}  // namespace asvrl
