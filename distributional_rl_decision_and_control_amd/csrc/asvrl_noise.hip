// asvrl_noise.hip -- one env step's perception noise from every robot's own numpy RandomState stream, continued
// on the device: asvrl_noise_streams, and its host twin asvrl_noise_streams_host on the same draw functions
// (asvrl_rs_stream.h).
//
// The work of a robot is one serial chain: about 17 MT19937 words per candidate, each accept / reject decision
// deciding where the next value starts, over a 2.5 KB state. Layout: one wave (a 64-thread workgroup) per robot
// row. The 624 key words are staged in LDS; every lane runs the same chain on the same words (LDS broadcast
// reads, wave-uniform control flow), so when the position reaches 624 the whole wave is at the regeneration and
// shares it, 64 words per pass; lane 0 alone stores the values into the row image in LDS. The wave then writes
// the row, zero padding included, and the key back with coalesced stores. A 64-lane f64 instruction costs what a
// 1-lane one does, so running the chain in every lane is free and spares the regeneration any divergence.
// A robot that does not draw (masked env, padding row, deactivated) only zeroes its row.
#include "asvrl_common.h"
#include "asvrl_rs_stream.h"

namespace asvrl {
namespace {

// mt19937_gen shared by the wave: pass b forms words [64 b, 64 b + 64) from values read before any of them is
// stored. Word i reads i + 1 (a later word of the same pass, or of a later one: still old, as the serial loop
// reads it; for i = 623 word 0, new in both) and i + 397 mod 624 (i < 227: old, written four or more passes on;
// else i - 227, new since an earlier pass because 227 > 64): the serial loop's values word for word.
struct RegenWave {
  __device__ static void run(uint32_t* key) {
    const int lane = threadIdx.x;
    for (int base = 0; base < kRsN; base += kWave) {
      const int i = base + lane;
      uint32_t v = 0;
      if (i < kRsN) {
        const int next = i + 1 < kRsN ? i + 1 : 0;
        const int far = i + kRsM < kRsN ? i + kRsM : i + kRsM - kRsN;
        v = rs_twist(key[i], key[next], key[far]);
      }
      __syncthreads();
      if (i < kRsN) key[i] = v;
      __syncthreads();
    }
  }
};

__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kWave) void noise_streams_kernel(const AsvNoiseStreams a, double pos_std,
                                                              double vel_std, double r_kappa) {
  __shared__ uint32_t skey[kRsN];
  extern __shared__ __attribute__((aligned(16))) double srow[];   // [O + R][5]
  const int lane = threadIdx.x;
  const int R = a.max_robots, O = a.max_obs;
  const int n5 = (O + R) * 5;
  const size_t row = blockIdx.x;
  const int e = static_cast<int>(row / R), i = static_cast<int>(row - static_cast<size_t>(e) * R);
  double* out = a.noise_out + row * n5;
  const int nrob = clampi(a.n_robots[e], 0, R), nobs = clampi(a.n_obs[e], 0, O);
  const bool draws = (a.env_mask == nullptr || a.env_mask[e] != 0) && i < nrob &&
                     (a.rflags[row] & ASVRL_FLAG_DEACTIVATED) == 0;
  if (!draws) {   // workgroup-uniform
    for (int k = lane; k < n5; k += kWave) out[k] = 0.0;
    return;
  }
  uint32_t* gkey = a.key + row * kRsN;
  for (int k = lane; k < kRsN; k += kWave) skey[k] = gkey[k];
  for (int k = lane; k < n5; k += kWave) srow[k] = 0.0;
  __syncthreads();
  if (a.robot_params != nullptr) {
    const AsvParams& P = a.robot_params[row];
    pos_std = P.pos_std;
    vel_std = P.vel_std;
    r_kappa = P.r_kappa;
  }
  RsStream s{skey, a.pos[row], a.has_gauss[row], a.gauss[row]};
  RsCounters c{0, 0.0, 0.0};
  if (a.draws_n != nullptr) c = RsCounters{a.draws_n[row], a.draws_sum[row], a.draws_sq[row]};
  rs_fill_row<RegenWave>(s, i, nrob, nobs, O, a.rflags + static_cast<size_t>(e) * R, pos_std, vel_std, r_kappa, c,
                         [&](int slot, int q, double v) {
                           if (lane == 0) srow[slot * 5 + q] = v;
                         });
  __syncthreads();
  for (int k = lane; k < n5; k += kWave) out[k] = srow[k];
  for (int k = lane; k < kRsN; k += kWave) gkey[k] = skey[k];
  if (lane == 0) {
    a.pos[row] = s.pos;
    a.has_gauss[row] = s.has_gauss;
    a.gauss[row] = s.gauss;
    if (a.draws_n != nullptr) {
      a.draws_n[row] = c.n;
      a.draws_sum[row] = c.sum;
      a.draws_sq[row] = c.sq;
    }
  }
}

int check_args(const std::string& who, const AsvParams* p, const AsvNoiseStreams* a) {
  ASVRL_REQUIRE(p != nullptr, who + ": null params");
  ASVRL_REQUIRE(a != nullptr, who + ": null struct");
  ASVRL_REQUIRE(a->n_envs >= 1, who + ": n_envs must be >= 1");
  ASVRL_REQUIRE(a->max_robots >= 1 && a->max_robots <= 256, who + ": max_robots must be in 1..256");
  ASVRL_REQUIRE(a->max_obs >= 0, who + ": max_obs must be >= 0");
  ASVRL_REQUIRE(a->max_obs + a->max_robots <= 1024, who + ": max_obs + max_robots must be <= 1024");
#define ASVRL_NOISE_ARRAY(name) ASVRL_REQUIRE(a->name != nullptr, who + ": null array " #name)
  ASVRL_NOISE_ARRAY(n_robots);
  ASVRL_NOISE_ARRAY(n_obs);
  ASVRL_NOISE_ARRAY(rflags);
  ASVRL_NOISE_ARRAY(key);
  ASVRL_NOISE_ARRAY(pos);
  ASVRL_NOISE_ARRAY(has_gauss);
  ASVRL_NOISE_ARRAY(gauss);
  ASVRL_NOISE_ARRAY(noise_out);
#undef ASVRL_NOISE_ARRAY
  const int counted = (a->draws_n != nullptr) + (a->draws_sum != nullptr) + (a->draws_sq != nullptr);
  ASVRL_REQUIRE(counted == 0 || counted == 3, who + ": draws_n, draws_sum and draws_sq go together (all or none)");
  return 0;
}

}  // namespace
}  // namespace asvrl

using namespace asvrl;

extern "C" int64_t asvrl_noise_streams_struct_size(void) { return sizeof(AsvNoiseStreams); }

extern "C" int asvrl_noise_streams(const AsvParams* p, const AsvNoiseStreams* ns, void* stream) {
  if (check_args("asvrl_noise_streams", p, ns)) return 1;
  const size_t NT = static_cast<size_t>(ns->n_envs) * ns->max_robots;
  ASVRL_REQUIRE(NT <= 0x7fffffffu, "asvrl_noise_streams: n_envs * max_robots must fit the grid");
  const size_t smem = static_cast<size_t>(ns->max_obs + ns->max_robots) * 5 * sizeof(double);
  hipLaunchKernelGGL(noise_streams_kernel, dim3(static_cast<unsigned>(NT)), dim3(kWave), smem, as_stream(stream), *ns,
                     p->pos_std, p->vel_std, p->r_kappa);
  return check_launch("asvrl_noise_streams");
}

extern "C" int asvrl_noise_streams_host(const AsvParams* p, const AsvNoiseStreams* ns, void* /*stream*/) {
  if (check_args("asvrl_noise_streams_host", p, ns)) return 1;
  const AsvNoiseStreams& a = *ns;
  const int R = a.max_robots, O = a.max_obs;
  const int n5 = (O + R) * 5;
  for (int e = 0; e < a.n_envs; ++e) {
    const int nrob = clampi(a.n_robots[e], 0, R), nobs = clampi(a.n_obs[e], 0, O);
    const bool env_on = a.env_mask == nullptr || a.env_mask[e] != 0;
    for (int i = 0; i < R; ++i) {
      const size_t row = static_cast<size_t>(e) * R + i;
      double* out = a.noise_out + row * n5;
      for (int k = 0; k < n5; ++k) out[k] = 0.0;
      if (!env_on || i >= nrob || (a.rflags[row] & ASVRL_FLAG_DEACTIVATED) != 0) continue;
      const AsvParams& P = a.robot_params != nullptr ? a.robot_params[row] : *p;
      RsStream s{a.key + row * kRsN, a.pos[row], a.has_gauss[row], a.gauss[row]};
      RsCounters c{0, 0.0, 0.0};
      if (a.draws_n != nullptr) c = RsCounters{a.draws_n[row], a.draws_sum[row], a.draws_sq[row]};
      rs_fill_row<RsRegenSerial>(s, i, nrob, nobs, O, a.rflags + static_cast<size_t>(e) * R, P.pos_std, P.vel_std,
                                 P.r_kappa, c, [&](int slot, int q, double v) { out[slot * 5 + q] = v; });
      a.pos[row] = s.pos;
      a.has_gauss[row] = s.has_gauss;
      a.gauss[row] = s.gauss;
      if (a.draws_n != nullptr) {
        a.draws_n[row] = c.n;
        a.draws_sum[row] = c.sum;
        a.draws_sq[row] = c.sq;
      }
    }
  }
  return 0;
}
