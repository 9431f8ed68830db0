// asvrl_actor_tile.h -- one 32-row tile of the AC-IQN Actor in one wave (AC_IQN_model.py:284-321): the
// observation encoders as one block-structured 256 x 32 matrix, hidden_layer 256 -> 128, hidden_layer_2
// 128 -> 128, output_layer 128 -> 2 with (2/pi) atan, and the epsilon-greedy draw of the batched act
// (agent.py:207-225). Shared by asvrl_mlp.hip (actor_kernel, encode_kernel) and asvrl_env.hip
// (env_policy_rollout_kernel, the Actor in front of every env step): the same MFMAs in the same order, so a row's
// action does not depend on which kernel computed it. asvrl_dqn.hip runs the same trunk (trunk_chain) under
// DQN_Policy's 25-wide head.
#pragma once
#include "asvrl_common.h"
#include "asvrl_mfma.h"
#include "asvrl_lds.h"

namespace asvrl {
namespace {
namespace atile {

constexpr int kEnc = 256, kObsK = 32, kHid = 128, kNa = 2;
constexpr int kSelfF = 56, kObjF = 40, kSelfIn = 7, kObjIn = 5, kObjN = 5;
constexpr int kFragEnc = kEnc * kObsK / 8;   // 1024 fragments
constexpr int kFragAe = kHid * 16 / 8;       // 256 (action encoder, K padded 2 -> 16)
constexpr int kFragH1 = kHid * kEnc / 8;     // 4096
constexpr int kFragH2 = kHid * kHid / 8;     // 2048

enum { MLP_ENCODE = 0, MLP_ACT = 1, MLP_FWD = 2, MLP_TRAIN = 3 };

struct MlpArgs {
  AsvMlpWeights w;
  AsvMlpIO io;
};

struct ActorLds {
  frag8 enc[lds_frags(kFragEnc)];
  frag8 w1[lds_frags(kFragH1)];
  frag8 w2[lds_frags(kFragH2)];
  float benc[kEnc], b1[kHid], b2[kHid], wout[kNa * kHid], bout[kNa];
};

// object index of encoder feature m (>= 56)
__host__ __device__ constexpr int obj_of(int m) { return (m - kSelfF) / kObjF; }

// Encoder output of one 32-row tile: B operand from obs columns 0..31, 8 blocks in 2 halves;
// epilogue bias + relu + mask. Hands each finished (block, s) group of 8 features to `emit`.
template <typename Emit>
__device__ __forceinline__ void encode_tile(const frag8* ENC, const float* benc, const frag8 (&bx)[2],
                                            const float (&mk)[kObjN], int lane, Emit emit) {
  const int h = lane >> 5;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x16{};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = mfma(ENC[((half * 4 + q) * 2 + ks) * 64 + lane], bx[ks], acc[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int mb = half * 4 + q;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int g = 8 * s + j;
          const int m0 = mb * 32 + (g & 3) + 8 * (g >> 2);   // feature for h = 0; h = 1 adds 4
          const float mk0 = m0 < kSelfF ? 1.f : (mk[obj_of(m0)] < 0.5f ? 0.f : 1.f);
          const float mk1 = m0 + 4 < kSelfF ? 1.f : (mk[obj_of(m0 + 4)] < 0.5f ? 0.f : 1.f);
          float x = acc[q][g] + benc[m0 + 4 * h];
          x = relu(x);
          v[j] = x * (h ? mk1 : mk0);
        }
        emit(mb, s, v);
      }
    }
  }
}

// bf16 B operand of the encoder (obs columns 0..31) + the object mask, for row `row`
__device__ __forceinline__ void load_obs(const float* __restrict__ x, int64_t ldx, int row, int h, frag8 (&bx)[2],
                                         float (&mk)[kObjN]) {
  const float* xr = x + static_cast<int64_t>(row) * ldx;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const float4 u = *reinterpret_cast<const float4*>(xr + ks * 16 + 8 * h);
    const float4 v = *reinterpret_cast<const float4*>(xr + ks * 16 + 8 * h + 4);
    const float e[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    bx[ks] = pack8(e);
  }
#pragma unroll
  for (int o = 0; o < kObjN; ++o) mk[o] = xr[32 + o];
}

// The Actor's weights into a workgroup's LDS with its T threads: the three images (bf16 build; the f32 build
// reads its fragments from L2, wimg) and the f32 biases and output layer. The caller's barrier follows.
template <int T>
__device__ __forceinline__ void stage_actor(ActorLds& L, const AsvMlpWeights& w, int tid) {
  const frag8* ge = reinterpret_cast<const frag8*>(w.enc_frag);
  const frag8* g1 = reinterpret_cast<const frag8*>(w.w1_frag);
  const frag8* g2 = reinterpret_cast<const frag8*>(w.w2_frag);
  if constexpr (kWeightsInLds) {
    constexpr int CH = kElemBytes == 2 ? 16 : 8;   // fragments in flight per thread
    copy_frags<T, kFragEnc, CH>(L.enc, ge, tid);
    copy_frags<T, kFragH1, CH>(L.w1, g1, tid);
    copy_frags<T, kFragH2, CH>(L.w2, g2, tid);
  }
  for (int i = tid; i < kEnc; i += T) L.benc[i] = w.b_enc[i];
  for (int i = tid; i < kHid; i += T) {
    L.b1[i] = w.b1[i];
    L.b2[i] = w.b2[i];
    L.wout[i] = w.wout[i];
    L.wout[kHid + i] = w.wout[kHid + i];
  }
  if (tid < kNa) L.bout[tid] = w.bout[tid];
}

// The forward chain of one tile: the lane's row (`row`, written only when `valid`) from its encoder operand
// to the pre-atan outputs (z0, z1) and the actions (a0, a1), in every lane of the row's pair (h = 0, 1).
// MLP_TRAIN saves the activations the backward reads.
// HEAD = false (trunk_chain below: DQN_Policy has the same trunk under another output layer, asvrl_dqn.hip):
// the chain stops behind hidden_layer_2 and leaves h2 in `h2v` -- element j of chained k-step group
// grp = 2 mb + s is feature feat(mb, 8 s + j, h), what a following layer's B operand packs; z and a are not
// written. The Actor's own instantiation is the same statements as before the split.
template <int MODE, bool HEAD = true>
__device__ __forceinline__ void actor_chain(const AsvMlpWeights& w, const AsvMlpIO& io, const ActorLds& L, int row,
                                            bool valid, int lane, const frag8 (&bx)[2], const float (&mk)[kObjN],
                                            float& z0, float& z1, float& a0, float& a1, float (*h2v)[8] = nullptr) {
  const int h = lane >> 5;
  // encoders -> h0 (chained B operand of hidden_layer)
  frag8 fpk[16];
  encode_tile(wimg(L.enc, w.enc_frag), L.benc, bx, mk, lane, [&](int mb, int s, const float* v) {
    fpk[mb * 2 + s] = pack8(*reinterpret_cast<const float (*)[8]>(v));
    if (MODE == MLP_TRAIN)
      store16(valid ? bp(io.h0) + static_cast<int64_t>(row) * kEnc + mb * 32 + 16 * s : nullptr, v, h);
  });
  // hidden_layer 256 -> 128, relu
  const frag8* W1 = wimg(L.w1, w.w1_frag);
  const frag8* W2 = wimg(L.w2, w.w2_frag);
  f32x16 acc1[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc1[mb] = f32x16{};
#pragma unroll
  for (int ks = 0; ks < kEnc / 16; ++ks)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc1[mb] = mfma(W1[(mb * 16 + ks) * 64 + lane], fpk[ks], acc1[mb]);
  frag8 h1pk[8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = acc1[mb][8 * s + j] + L.b1[feat(mb, 8 * s + j, h)];
        v[j] = relu(x);
      }
      h1pk[mb * 2 + s] = pack8(v);
      if (MODE == MLP_TRAIN)
      store16(valid ? bp(io.h1) + static_cast<int64_t>(row) * kHid + mb * 32 + 16 * s : nullptr, v, h);
    }
  // hidden_layer_2 128 -> 128, relu; output_layer 128 -> 2
  f32x16 acc2[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc2[mb] = f32x16{};
#pragma unroll
  for (int ks = 0; ks < kHid / 16; ++ks)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc2[mb] = mfma(W2[(mb * 8 + ks) * 64 + lane], h1pk[ks], acc2[mb]);
  float p0 = 0.f, p1 = 0.f;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = feat(mb, 8 * s + j, h);
        const float x = acc2[mb][8 * s + j] + L.b2[m];
        v[j] = relu(x);
        if constexpr (HEAD) {
          p0 += L.wout[m] * v[j];
          p1 += L.wout[kHid + m] * v[j];
        } else {
          h2v[mb * 2 + s][j] = v[j];
        }
      }
      if (MODE == MLP_TRAIN)
      store16(valid ? bp(io.h2) + static_cast<int64_t>(row) * kHid + mb * 32 + 16 * s : nullptr, v, h);
    }
  if constexpr (HEAD) {
    z0 = p0 + __shfl_xor(p0, 32, 64) + L.bout[0];
    z1 = p1 + __shfl_xor(p1, 32, 64) + L.bout[1];
    a0 = w.out_scale * atanf(z0);   // atan_scale * torch.atan(actions)
    a1 = w.out_scale * atanf(z1);
  }
}

// The trunk alone: h2 of the lane's row as the eight chained k-step groups of a following layer's B operand.
template <int MODE>
__device__ __forceinline__ void trunk_chain(const AsvMlpWeights& w, const AsvMlpIO& io, const ActorLds& L, int row,
                                            bool valid, int lane, const frag8 (&bx)[2], const float (&mk)[kObjN],
                                            float (&h2v)[8][8]) {
  float z0, z1, a0, a1;   // not written with HEAD = false
  actor_chain<MODE, false>(w, io, L, row, valid, lane, bx, mk, z0, z1, a0, a1, h2v);
}

// epsilon-greedy (agent.py:207-225): greedy iff random() > eps, else uniform(-1, 1) per dim; eps: linear
// schedule of the step count (trainer.py:257-264). The draw is keyed by (row, step) and the policy's seed.
struct EpsSchedule {
  double steps_per_count, total, fraction, eps_initial, eps_final;
};
__device__ __forceinline__ void explore(uint64_t step, const EpsSchedule& s, uint64_t seed, int row, float a0,
                                        float a1, double& o0, double& o1) {
  const double progress = static_cast<double>(step) * s.steps_per_count / s.total;
  const double eps = progress < s.fraction ? s.eps_initial + (progress / s.fraction) * (s.eps_final - s.eps_initial)
                                            : s.eps_final;
  const U4 u = philox4x32_10(U4{static_cast<uint32_t>(row), static_cast<uint32_t>(step),
                                static_cast<uint32_t>(step >> 32), 0xAC7u},
                             static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  const double c = (static_cast<double>(u.x >> 8) + 1.0) * (1.0 / 16777216.0);   // (0, 1]
  if (c > eps) {
    o0 = a0;
    o1 = a1;
  } else {
    o0 = 2.0 * (static_cast<double>(u.y >> 8) * (1.0 / 16777216.0)) - 1.0;
    o1 = 2.0 * (static_cast<double>(u.z >> 8) * (1.0 / 16777216.0)) - 1.0;
  }
}

}  // namespace atile
}  // namespace
}  // namespace asvrl
