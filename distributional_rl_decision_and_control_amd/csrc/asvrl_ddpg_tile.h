// asvrl_ddpg_tile.h -- DDPG_model.Critic on the one-wave Actor tile (asvrl_actor_tile.h): one scalar Q per row.
// The chain is the Actor's up to hidden_layer (encode_tile, the same W1 MFMAs), then the product with the action
// features G = relu(Wae a + bae) -- computed per lane in f32 from the row's two action inputs, two multiplies and
// two adds per feature, no MFMA -- hidden_layer_2 on p = h1 * G and the 128 -> 1 output layer as a per-lane dot
// product closed by one exchange between the lane halves. Shared by the three kernels of asvrl_ddpg.hip.
#pragma once
#include "asvrl_actor_tile.h"

namespace asvrl {
namespace {
namespace ddtile {
using namespace atile;

enum { DD_FWD = 0, DD_TRAIN = 1, DD_ACTOR = 2 };

// the action encoder in LDS: weight [128][2], then bias [128]
struct AeLds {
  float w[kHid * kNa], b[kHid];
};

// The action encoder of `w` into LDS with the workgroup's T threads (the caller's barrier follows).
template <int T>
__device__ __forceinline__ void stage_ae(AeLds& A, const AsvDdpgWeights& w, int tid) {
  for (int i = tid; i < kHid * kNa; i += T) A.w[i] = w.wae[i];
  for (int i = tid; i < kHid; i += T) A.b[i] = w.bae[i];
}

// G[m] = relu(Wae[m] . a + bae[m]): the dot product first, the bias after it (torch's addmm order)
__device__ __forceinline__ float ae_feature(const float* wae, const float* bae, int m, float a0, float a1) {
  return relu((wae[2 * m] * a0 + wae[2 * m + 1] * a1) + bae[m]);
}

// What the actor step keeps of the forward for its backward: t = h1 1[G > 0] (dzG = dp t) in accumulator order
// (t[mb][g] <-> feat(mb, g, h)) and dz2 = dq wo 1[z2 > 0] as the chained B operand of W2^T.
struct ActorKeep {
  float t[4][16];
  frag8 dz2pk[8];
};

// Q of the lane's row (both lanes of the row's pair end with it). a0, a1: the row's action. MODE DD_TRAIN saves
// xb / h0 / h1 / p / h2 into `io` (written only when `valid`); DD_ACTOR fills `keep` for output gradient `dq`.
template <int MODE>
__device__ __forceinline__ float ddpg_q_tile(const AsvMlpWeights& w, const AsvDdpgGradIO& io, const ActorLds& L,
                                             const AeLds& A, int row, bool valid, int lane, const frag8 (&bx)[2],
                                             const float (&mk)[kObjN], float a0, float a1, float dq = 0.f,
                                             ActorKeep* keep = nullptr) {
  const int h = lane >> 5;
  if (MODE == DD_TRAIN && valid) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      *reinterpret_cast<frag8*>(bp(io.xb) + static_cast<int64_t>(row) * kObsK + ks * 16 + 8 * h) = bx[ks];
  }
  // encoders -> F (chained B operand of hidden_layer)
  frag8 fpk[16];
  encode_tile(wimg(L.enc, w.enc_frag), L.benc, bx, mk, lane, [&](int mb, int s, const float* v) {
    fpk[mb * 2 + s] = pack8(*reinterpret_cast<const float (*)[8]>(v));
    if (MODE == DD_TRAIN)
      store16(valid ? bp(io.h0) + static_cast<int64_t>(row) * kEnc + mb * 32 + 16 * s : nullptr, v, h);
  });
  // hidden_layer 256 -> 128, relu, times G
  const frag8* W1 = wimg(L.w1, w.w1_frag);
  const frag8* W2 = wimg(L.w2, w.w2_frag);
  f32x16 acc1[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc1[mb] = f32x16{};
#pragma unroll
  for (int ks = 0; ks < kEnc / 16; ++ks)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc1[mb] = mfma(W1[(mb * 16 + ks) * 64 + lane], fpk[ks], acc1[mb]);
  frag8 ppk[8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float hv[8], pv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = feat(mb, 8 * s + j, h);
        hv[j] = relu(acc1[mb][8 * s + j] + L.b1[m]);
        const float g = ae_feature(A.w, A.b, m, a0, a1);
        pv[j] = hv[j] * g;
        if (MODE == DD_ACTOR) keep->t[mb][8 * s + j] = g > 0.f ? hv[j] : 0.f;
      }
      ppk[mb * 2 + s] = pack8(pv);
      if (MODE == DD_TRAIN) {
        store16(valid ? bp(io.h1) + static_cast<int64_t>(row) * kHid + mb * 32 + 16 * s : nullptr, hv, h);
        store16(valid ? bp(io.p) + static_cast<int64_t>(row) * kHid + mb * 32 + 16 * s : nullptr, pv, h);
      }
    }
  // hidden_layer_2 128 -> 128, relu; output_layer 128 -> 1
  f32x16 acc2[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc2[mb] = f32x16{};
#pragma unroll
  for (int ks = 0; ks < kHid / 16; ++ks)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc2[mb] = mfma(W2[(mb * 8 + ks) * 64 + lane], ppk[ks], acc2[mb]);
  float part = 0.f;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float v[8], dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = feat(mb, 8 * s + j, h);
        v[j] = relu(acc2[mb][8 * s + j] + L.b2[m]);
        part += L.wout[m] * v[j];
        if (MODE == DD_ACTOR) dv[j] = v[j] > 0.f ? L.wout[m] * dq : 0.f;
      }
      if (MODE == DD_ACTOR) keep->dz2pk[mb * 2 + s] = pack8(dv);
      if (MODE == DD_TRAIN)
        store16(valid ? bp(io.h2) + static_cast<int64_t>(row) * kHid + mb * 32 + 16 * s : nullptr, v, h);
    }
  return part + __shfl_xor(part, 32, 64) + L.bout[0];   // every lane of the wave is live here
}

}  // namespace ddtile
}  // namespace
}  // namespace asvrl
