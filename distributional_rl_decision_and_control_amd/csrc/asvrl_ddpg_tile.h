// asvrl_ddpg_tile.h -- DDPG_model.Critic on the one-wave Actor tile (asvrl_actor_tile.h): one scalar Q per row.
// The chain is the Actor's up to hidden_layer (encode_tile, the same W1 MFMAs), then the product with the action
// features G = relu(Wae a + bae) -- computed per lane in f32 from the row's two action inputs, two multiplies and
// two adds per feature, no MFMA -- hidden_layer_2 on p = h1 * G and the 128 -> 1 output layer as a per-lane dot
// product closed by one exchange between the lane halves. Shared by the three kernels of asvrl_ddpg.hip and by SAC's twin critics
// (asvrl_sac.hip), with the backward behind dq (ddpg_bwd_tile) and the action gradient (ddpg_dA_tile).
#pragma once
#include "asvrl_actor_tile.h"

namespace asvrl {
namespace {
namespace ddtile {
using namespace atile;

enum { DD_FWD = 0, DD_TRAIN = 1, DD_ACTOR = 2 };
constexpr int kActCol = 2 * ASVRL_OBS_DIM;   // replay row: action (2), reward, done behind s and s'

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

// 16 saved activations of block mb of the lane's row in accumulator order (register g <-> feat(mb, g, h))
__device__ __forceinline__ void ddpg_load16(const elem_t* rowp, int mb, int h, float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 16; g += 4) load4(rowp + mb * 32 + 8 * (g >> 2) + 4 * h, &v[g]);
}

// The critic's backward behind the output layer's gradient dq of the lane's row (rr; stores only when `valid`): dz2,
// dz1, dzG and dz0 = dzF from the saved h2 / h1 / h0 of `io`, by W2^T and W1^T of `w` (read from L2). a0, a1: the
// row's action. No LDS, no barrier. Shared by ddpg_bwd_kernel and SAC's twin backward (asvrl_sac.hip).
__device__ __forceinline__ void ddpg_bwd_tile(const AsvDdpgWeights& w, const AsvDdpgGradIO& io, int lane, int64_t rr,
                                              bool valid, float a0, float a1, float dq) {
  const int h = lane >> 5;
  // ---------------- dz2 = dq wo 1[z2 > 0]
  const float* wo = w.trunk.wout;
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
  const frag8* W2T = reinterpret_cast<const frag8*>(w.trunk.w2t_frag);
  const frag8* W1T = reinterpret_cast<const frag8*>(w.trunk.w1t_frag);
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
        const float g = ae_feature(w.wae, w.bae, feat(mb, 8 * s + j, h), a0, a1);
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

// dA = Wae^T dzG of the lane's row from what a DD_ACTOR pass kept: dp = W2^T dz2, dzG = dp h1 1[G > 0]. Every lane
// of the wave must be live (one exchange between the lane halves); both lanes of the row's pair end with (d0, d1).
__device__ __forceinline__ void ddpg_dA_tile(const AsvDdpgWeights& w, const AeLds& A, const ActorKeep& keep, int lane,
                                             float& d0, float& d1) {
  const int h = lane >> 5;
  // dp = W2^T dz2; dzG = dp h1 1[G > 0]; dA = Wae^T dzG
  const frag8* W2T = reinterpret_cast<const frag8*>(w.trunk.w2t_frag);
  d0 = 0.f;
  d1 = 0.f;
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
}

}  // namespace ddtile

// Host side: the images a critic launch reads, by name ("<who>: null array <name>.<field>"); backward: W2^T and W1^T too.
inline int ddpg_check_weights(const std::string& who, const char* name, const AsvDdpgWeights* w, bool backward) {
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
