// asvrl_rs_stream.h -- numpy's legacy RandomState stream (MT19937, the polar-method normal, Best & Fisher's
// von Mises) as __host__ __device__ functions: the draws each robot's Perception makes from
// numpy.random.RandomState(seed) (wamv.py:5-40), reproduced word for word so that a stream state taken from
// RandomState.get_state() continues on the device where numpy would have continued on the host.
//
// A stream is {key[624], pos, has_gauss, gauss} (numpy's get_state() tuple). RsStream holds the scalars by value
// and points at the key words, which live wherever the caller keeps them (host memory, or a workgroup's LDS).
// Regen::run(key) is the caller's regeneration of the 624 words (rs_regen_serial here; a wave-cooperative one in
// asvrl_noise.hip); everything else is shared, so the host twin and the kernel run the same arithmetic. The file is
// compiled with -ffp-contract=off: numpy's build contracts no product into an FMA either.
//
// The rejection loops are numpy's, with one addition: each gives up after kRsMaxTries rounds. A seeded MT19937
// state passes the normal's loop with probability pi / 4 per round and the von Mises loop with more, so a valid
// stream never gets there; an all-zero (never initialised) key would otherwise spin for ever.
#pragma once

#include <cmath>
#include <cstdint>

namespace asvrl {

constexpr int kRsN = 624, kRsM = 397;
constexpr int kRsMaxTries = 1024;
constexpr double kRsPi = 3.14159265358979323846;   // M_PI

struct RsStream {
  uint32_t* key;   // [624]
  int32_t pos;
  int32_t has_gauss;
  double gauss;
};

// count, sum and sum of squares of the values drawn, in draw order
struct RsCounters {
  int64_t n;
  double sum, sq;
};

__host__ __device__ inline uint32_t rs_twist(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// mt19937_gen: the next 624 words, in place
struct RsRegenSerial {
  __host__ __device__ static void run(uint32_t* key) {
    int i = 0;
    for (; i < kRsN - kRsM; ++i) key[i] = rs_twist(key[i], key[i + 1], key[i + kRsM]);
    for (; i < kRsN - 1; ++i) key[i] = rs_twist(key[i], key[i + 1], key[i + (kRsM - kRsN)]);
    key[kRsN - 1] = rs_twist(key[kRsN - 1], key[0], key[kRsM - 1]);
  }
};

template <class Regen>
__host__ __device__ inline uint32_t rs_word(RsStream& s) {
  if (s.pos < 0 || s.pos >= kRsN) {   // numpy: pos == 624 (a state from get_state() holds 0..624)
    Regen::run(s.key);
    s.pos = 0;
  }
  uint32_t y = s.key[s.pos++];
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// random_sample's 53-bit double in [0, 1) from two consecutive words
template <class Regen>
__host__ __device__ inline double rs_double(RsStream& s) {
  const uint32_t a = rs_word<Regen>(s) >> 5;
  const uint32_t b = rs_word<Regen>(s) >> 6;
  return (a * 67108864.0 + b) / 9007199254740992.0;
}

// legacy_gauss: Marsaglia's polar method, the second value of a pair cached
template <class Regen>
__host__ __device__ inline double rs_gauss(RsStream& s) {
  if (s.has_gauss) {
    const double v = s.gauss;
    s.has_gauss = 0;
    s.gauss = 0.0;
    return v;
  }
  double x1 = 0.0, x2 = 0.0, r2 = 0.0;
  for (int it = 0; it < kRsMaxTries; ++it) {
    x1 = 2.0 * rs_double<Regen>(s) - 1.0;
    x2 = 2.0 * rs_double<Regen>(s) - 1.0;
    r2 = x1 * x1 + x2 * x2;
    if (r2 < 1.0 && r2 != 0.0) break;
  }
  const double f = sqrt(-2.0 * log(r2) / r2);
  s.gauss = f * x1;
  s.has_gauss = 1;
  return f * x2;
}

template <class Regen>
__host__ __device__ inline double rs_normal(RsStream& s, double loc, double scale) {
  return loc + scale * rs_gauss<Regen>(s);
}

// RandomState.vonmises (legacy_vonmises). The envelope parameter is formed as numpy forms it, through rho (and the
// second-order expansion below kappa = 1e-5): 0.5 / kappa + sqrt(1 + (0.5 / kappa)^2) is the same number on paper and
// the same double at the default kappa = 1, but a last-bit neighbour at most other kappas, which moves the draws.
template <class Regen>
__host__ __device__ inline double rs_vonmises(RsStream& s, double mu, double kappa) {
  if (kappa < 1e-8) return kRsPi * (2 * rs_double<Regen>(s) - 1);
  double r;
  if (kappa < 1e-5) {
    r = 1. / kappa + kappa;
  } else {
    const double q = 1 + sqrt(1 + 4 * kappa * kappa);
    const double rho = (q - sqrt(2 * q)) / (2 * kappa);
    r = (1 + rho * rho) / (2 * rho);
  }
  double W = 1.0;
  for (int it = 0; it < kRsMaxTries; ++it) {
    const double U = rs_double<Regen>(s);
    const double Z = cos(kRsPi * U);
    W = (1 + r * Z) / (r + Z);
    const double Y = kappa * (r - W);
    const double V = rs_double<Regen>(s);
    if ((Y * (2 - Y) - V >= 0) || (log(Y / V) + 1 - Y >= 0)) break;
  }
  const double U = rs_double<Regen>(s);
  double res = acos(W);
  if (U < 0.5) res = -res;
  res += mu;
  const bool neg = res < 0;
  double m = fabs(res);
  m = fmod(m + kRsPi, 2 * kRsPi) - kRsPi;
  if (neg) m = -m;
  return m;
}

// Perception.draw_candidate_noise: two position normals, two velocity normals, the radius' von Mises draw.
// put(k, v) stores value k of the candidate.
template <class Regen, class Put>
__host__ __device__ inline void rs_candidate(RsStream& s, double pos_std, double vel_std, double r_kappa,
                                             RsCounters& c, Put put) {
  double v[5];
  v[0] = rs_normal<Regen>(s, 0.0, pos_std);
  v[1] = rs_normal<Regen>(s, 0.0, pos_std);
  v[2] = rs_normal<Regen>(s, 0.0, vel_std);
  v[3] = rs_normal<Regen>(s, 0.0, vel_std);
  v[4] = rs_vonmises<Regen>(s, 0.0, r_kappa);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    put(k, v[k]);
    c.n += 1;
    c.sum += v[k];
    c.sq += v[k] * v[k];
  }
}

// One step's noise row of robot i of an env with nrob robots and nobs obstacles, in MarineNavEnv3._pack's order
// (wamv.py:465-510): slot k < nobs the obstacle k, slot O + j the robot j != i that is not deactivated. flags: the
// env's [nrob] robot flags. put(slot, k, v) stores a value; slots without a candidate are not touched (the caller
// zeroes the row). The caller has established that robot i draws at all.
template <class Regen, class Put>
__host__ __device__ inline void rs_fill_row(RsStream& s, int i, int nrob, int nobs, int O, const uint8_t* flags,
                                            double pos_std, double vel_std, double r_kappa, RsCounters& c, Put put) {
  for (int k = 0; k < nobs; ++k)
    rs_candidate<Regen>(s, pos_std, vel_std, r_kappa, c, [&](int q, double v) { put(k, q, v); });
  for (int j = 0; j < nrob; ++j) {
    if (j == i || (flags[j] & ASVRL_FLAG_DEACTIVATED)) continue;
    rs_candidate<Regen>(s, pos_std, vel_std, r_kappa, c, [&](int q, double v) { put(O + j, q, v); });
  }
}

}  // namespace asvrl
