// asvrl_eval.hip -- the evaluation bookkeeping of Trainer.evaluation (trainer.py:286-303) over the records of
// one hold_done rollout window: asvrl_eval_metrics; and, further down, its per-robot histories (trainer.py:347-365)
// cut out of episode-long records: asvrl_eval_history_count, asvrl_eval_history_pack; and, at the end, the return-to-go and
// calibration of recorded return distributions: asvrl_eval_dist_stats.
//
// The rollout kernels end an episode by the training rule (every robot deactivated, or the step limit). The
// evaluation rule also ends it at the first collision of any robot, and it accumulates, per robot that is not yet
// deactivated, the discounted return, the time dt * N and the energy of the thrusts after the step. This kernel
// folds a window's records (reward, info, the thrust planes of rs) into that state, carried from window to
// window; rows an env wrote after its evaluation end are ignored.
//
// Layout: one lane per robot row, floor(64 / max_robots) envs per wave, so a wave reads consecutive rows of the
// [K][NT] record planes. The per-env decision (any collision, all deactivated) is a __ballot over the wave,
// masked to the env's lanes. Every lane of an env carries the same length / ended in registers; its first lane
// stores them. No LDS, no atomics, no barrier: the step loop's trip count and its early exit are wave-uniform.
#include "asvrl_common.h"

namespace asvrl {
namespace {

__global__ __launch_bounds__(256) void eval_metrics_kernel(const AsvEvalMetrics m) {
  const int R = m.max_robots, E = m.n_envs, K = m.n_steps;
  const size_t NT = static_cast<size_t>(E) * R;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  const int epw = kWave / R;   // envs per wave
  const int le = lane / R, j = lane - le * R;
  const long long e64 = static_cast<long long>(wave) * epw + le;
  const bool valid = le < epw && e64 < E;
  const int e = valid ? static_cast<int>(e64) : 0;
  const size_t row = static_cast<size_t>(e) * R + j;
  // the lanes of this lane's env (R <= 32, so the shift stays inside 64 bits for every le < epw)
  const unsigned long long gm = valid ? (((1ull << R) - 1ull) << (le * R)) : 0ull;

  const bool exists = valid && j < m.n_robots[e];
  const int sr = valid ? min(m.steps_run[e], K) : 0;
  int length = valid ? m.length[e] : 0;
  bool ended = valid ? m.ended[e] != 0 : true;
  bool deact = exists ? m.deact[row] != 0 : true;
  uint8_t outcome = exists ? m.outcome[row] : 0;
  double ret = 0.0, tim = 0.0, en = 0.0, dt = 0.0, Nn = 0.0, pc = 0.0;
  if (exists) {
    ret = m.ret[row];
    tim = m.time[row];
    en = m.energy[row];
    dt = m.dt[row];
    Nn = m.N[row];
    pc = m.pc[row];
  }

  for (int t = 0; t < K; ++t) {
    const bool run = valid && !ended && t < sr;
    if (__ballot(run) == 0ull) break;   // wave-uniform: no env of this wave has a step left in the window
    bool coll = false;
    if (run && exists && !deact) {
      const size_t at = static_cast<size_t>(t) * NT + row;
      const size_t plane = static_cast<size_t>(t) * ASVRL_NUM_FIELDS * NT + row;
      const double rew = m.reward[at];
      const uint8_t info = m.info[at];
      const double tl = m.rs[plane + ASVRL_F_TL * NT], tr = m.rs[plane + ASVRL_F_TR * NT];
      ret += pow(m.gamma, static_cast<double>(length)) * rew;
      tim += dt * Nn;
      const double el = pc * fabs(tl) * dt * Nn;   // Robot.compute_step_energy_cost, left to right
      const double er = pc * fabs(tr) * dt * Nn;
      en += el + er;
      if (info == ASVRL_INFO_COLLISION) {
        coll = true;
        outcome = 2;
        deact = true;
      } else if (info == ASVRL_INFO_REACH_GOAL) {
        outcome = 1;
        deact = true;
      }
    }
    const unsigned long long collided = __ballot(coll);
    const unsigned long long active = __ballot(exists && !deact);
    if (run) {
      const bool end = (length >= m.episode_limit) || (collided & gm) != 0ull || (active & gm) == 0ull;
      length += 1;
      ended = end;
    }
  }

  if (exists) {
    m.deact[row] = deact ? 1 : 0;
    m.outcome[row] = outcome;
    m.ret[row] = ret;
    m.time[row] = tim;
    m.energy[row] = en;
  }
  if (valid && j == 0) {
    m.length[e] = length;
    m.ended[e] = ended ? 1 : 0;
    m.alive[e] = ended ? 0 : 1;
  }
}

// ------------------------------------------------------------------ episode histories
// asvrl_eval_history_count / asvrl_eval_history_pack: the observation, action and trajectory histories of
// Trainer.evaluation (trainer.py:347-365) cut out of episode-long records.
//
// count: one lane per robot row, as above; a wave reads consecutive bytes of one info row per step.
//
// pack: a masked transpose. The records are contiguous across robot rows for a fixed (step, field); a robot's history
// is contiguous across (step, field). A block of 256 threads takes kRows = 32 robot rows by kSteps = 16 history
// entries and moves each of the three transposed arrays through one LDS tile, the tile re-used between them:
//   trajectory  tile[16 * 13][33] f64. In: lane = row, 8 (entry, field) planes per pass, so a half-wave reads 32
//               consecutive doubles; ds_write_b64 (bank (a/4) % 32, groups of 16 consecutive lanes) sees 16
//               consecutive doubles = 32 banks. Out: a wave per robot row, lane = (entry, field) index p, consecutive
//               doubles in HBM; ds_read_b64 (bank (a/4) % 64, groups of 32 lanes) reads tile[p][row] at dword
//               2 * (33 p + row): 33 is odd, so 32 consecutive p land on the 32 even bank pairs once each.
//   actions     tile[16][66] f64, the (row, component) pairs of one step contiguous. In: a wave per step reads 64
//               consecutive doubles. Out: a half-wave per robot row, lane = (step, component); dword
//               2 * (66 s + 2 row + c) = 4 s + 2 c + const mod 64: 32 lanes, 32 bank pairs.
//   counts      tile[16][34] i32 (the i8 widened). In: lane = row, ds_write_b32 on consecutive dwords. Out: 16 lanes
//               per robot row, lane = entry: ds_read_b32 (bank (a/4) % 32) at dword 34 s + row: a half-wave holds two
//               rows, 2 s + row and 2 s + row + 1, 32 banks.
// The observation rows need no transpose: the packed row of a (step, robot) is 160 contiguous bytes of which the
// first 128 are kept, and a robot's consecutive entries are consecutive 128-byte rows of the output. Eight lanes
// move one row as float4, consecutive lane groups take consecutive entries of one robot.
// Per row the three counts bound every read and write; a tile with no entry below any of its rows' counts leaves
// after reading the counts.
constexpr int kHistRows = ASVRL_HISTORY_ROW_TILE, kHistSteps = ASVRL_HISTORY_STEP_TILE;
constexpr int kTrajDim = ASVRL_TRAJ_DIM, kHistObs = ASVRL_HISTORY_OBS_DIM;
constexpr int kTrajLd = kHistRows + 1, kActLd = 2 * kHistRows + 2, kCntLd = kHistRows + 2;
static_assert(kHistRows == 32 && kHistSteps == 16, "the lane maps below are written for a 32 x 16 tile");

__global__ __launch_bounds__(256) void eval_history_count_kernel(const AsvEvalHistory h) {
  const int R = h.max_robots, T = h.n_steps;
  const size_t NT = static_cast<size_t>(h.n_envs) * R;
  const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (row >= NT) return;
  const int e = static_cast<int>(row / R), j = static_cast<int>(row - static_cast<size_t>(e) * R);
  int n_traj = 0, n_act = 0, n_obs = 0;
  if (j < h.n_robots[e]) {
    const int L = min(max(h.length[e], 0), T);
    n_act = L;
    for (int s = 0; s < L; ++s) {
      const uint8_t info = h.info[static_cast<size_t>(s) * NT + row];
      if (info == ASVRL_INFO_COLLISION || info == ASVRL_INFO_REACH_GOAL) {
        n_act = s + 1;
        break;
      }
    }
    n_traj = n_act + 1;
    n_obs = L + 1;
  }
  h.counts[row] = n_traj;
  h.counts[NT + row] = n_act;
  h.counts[2 * NT + row] = n_obs;
}

__global__ __launch_bounds__(256) void eval_history_pack_kernel(const AsvEvalHistory h) {
  __shared__ double tile[kHistSteps * kTrajDim * kTrajLd];
  __shared__ int s_n[3][kHistRows];
  __shared__ long long s_off[3][kHistRows];
  const int T = h.n_steps;
  const size_t NT = static_cast<size_t>(h.n_envs) * h.max_robots;
  const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const size_t row0 = static_cast<size_t>(blockIdx.x) * kHistRows;
  const int k0 = blockIdx.y * kHistSteps;   // the tile's first history entry

  // the rows' counts, clamped to what the records hold and to the outputs' capacity
  int any = 0;
  if (t < 3 * kHistRows) {
    const int q = t / kHistRows, r = t - q * kHistRows;
    int n = 0;
    long long off = 0;
    if (row0 + r < NT) {
      n = h.counts[q * NT + row0 + r];
      off = h.offsets[q * NT + row0 + r];
      const long long cap = q == 0 ? h.traj_rows : (q == 1 ? h.act_rows : h.obs_rows);
      n = min(n, q == 1 ? min(T, h.act_steps) : T + 1);
      if (off < 0 || off > cap) n = 0;
      n = static_cast<int>(min(static_cast<long long>(n), cap - off));
      n = max(n, 0);
    }
    s_n[q][r] = n;
    s_off[q][r] = off;
    any = n > k0;
  }
  if (__syncthreads_or(any) == 0) return;

  // ---- trajectory: entry k of a row is rs0 (k = 0) or rs[k - 1], 13 of the 17 planes in wamv.py:191-193 order
  {
    const int r = t & (kHistRows - 1);
    const int lim = s_n[0][r] - k0;   // entries of this row inside the tile
    for (int p = t / kHistRows; p < kHistSteps * kTrajDim; p += 256 / kHistRows) {
      const int ks = p / kTrajDim, c = p - ks * kTrajDim;
      if (ks < lim) {
        const int f = c < ASVRL_F_TL ? c : (c < ASVRL_F_TL + 2 ? c + 2 : c - 2);   // ..., LP, RP, TL, TR
        const int k = k0 + ks;
        const double* src = k == 0 ? h.rs0 : h.rs + static_cast<size_t>(k - 1) * ASVRL_NUM_FIELDS * NT;
        tile[p * kTrajLd + r] = src[static_cast<size_t>(f) * NT + row0 + r];
      }
    }
    __syncthreads();
    for (int rr = wave; rr < kHistRows; rr += 256 / kWave) {
      const int n = min(s_n[0][rr] - k0, kHistSteps) * kTrajDim;
      double* dst = h.traj + (s_off[0][rr] + k0) * kTrajDim;
      for (int p = lane; p < n; p += kWave) dst[p] = tile[p * kTrajLd + rr];
    }
    __syncthreads();
  }

  // ---- actions: entry k is actions[k]
  {
    for (int ks = wave; ks < kHistSteps; ks += 256 / kWave) {
      const int r = lane >> 1;
      if (ks < s_n[1][r] - k0)
        tile[ks * kActLd + lane] = h.actions[(static_cast<size_t>(k0 + ks) * NT + row0) * 2 + lane];
    }
    __syncthreads();
    const int half = t >> 5, p = t & 31;   // (step, component) of one row per half-wave
    for (int rr = half; rr < kHistRows; rr += 256 / 32) {
      const int n = min(s_n[1][rr] - k0, kHistSteps) * 2;
      if (p < n) h.act[(s_off[1][rr] + k0) * 2 + p] = tile[(p >> 1) * kActLd + 2 * rr + (p & 1)];
    }
    __syncthreads();
  }

  // ---- object counts: entry k is cnt0 (k = 0) or obj_cnt[k - 1]
  {
    int* ctile = reinterpret_cast<int*>(tile);
    const int r = t & (kHistRows - 1);
    for (int ks = t / kHistRows; ks < kHistSteps; ks += 256 / kHistRows) {
      if (ks < s_n[2][r] - k0) {
        const int k = k0 + ks;
        ctile[ks * kCntLd + r] = k == 0 ? h.cnt0[row0 + r] : h.obj_cnt[static_cast<size_t>(k - 1) * NT + row0 + r];
      }
    }
    __syncthreads();
    const int ks = t & (kHistSteps - 1);
    for (int rr = t / kHistSteps; rr < kHistRows; rr += 256 / kHistSteps)
      if (ks < s_n[2][rr] - k0) h.cnt_out[s_off[2][rr] + k0 + ks] = static_cast<int8_t>(ctile[ks * kCntLd + rr]);
  }

  // ---- observations: 8 lanes per (row, entry), 16 bytes each
  {
    const int sub = t & 7;
    for (int pair = t >> 3; pair < kHistRows * kHistSteps; pair += 256 / 8) {
      const int rr = pair / kHistSteps, ks = pair - rr * kHistSteps;
      if (ks < s_n[2][rr] - k0) {
        const int k = k0 + ks;
        const float* src = k == 0 ? h.obs0 : h.obs + static_cast<size_t>(k - 1) * NT * ASVRL_OBS_DIM;
        const float4 v = reinterpret_cast<const float4*>(src + (row0 + rr) * ASVRL_OBS_DIM)[sub];
        reinterpret_cast<float4*>(h.obs_out + (s_off[2][rr] + k) * kHistObs)[sub] = v;
      }
    }
  }
}

// ------------------------------------------------------------------ return distributions
// asvrl_eval_dist_stats: the return-to-go of every robot and how the recorded quantile samples sit around it (the
// formulas stand at AsvEvalDistStats). Two launches:
//
// scan:  one lane per robot row, as the count kernel. G_t = reward[t] + gamma * G_{t+1} backwards from t = A - 1, one
//        dependent f64 multiply-add pair per step (uncontracted), G written to g_plane; a wave reads consecutive
//        doubles of one reward row per step. g0 and steps leave here.
// stats: one wave per robot row, lane = (step parity, sample): the two halves take the steps 2 i and 2 i + 1, which
//        depend on nothing but g_plane, so the loads of a pair are independent of every sum. Per step the three sums
//        over the 32 samples -- the count of z <= G, the pinball terms, z itself -- are the xor butterfly 16, 8, 4, 2,
//        1 inside the half, in f64 (every lane of the half ends with the same bits; the count is a ballot). Over the
//        steps each sum runs in lane 0 in the order t = 0, 1, 2, ...: step 2 i, then step 2 i + 1 (read from lane
//        32). The PIT bin u is counted by lane u (33 lanes, integers). No LDS, no atomics, no barrier; a robot's wave
//        does not know the block it sits in, so the block size changes nothing.
constexpr int kDistS = ASVRL_DIST_SAMPLES, kPitBins = kDistS + 1;
static_assert(2 * kDistS == kWave, "the stats kernel puts two steps of 32 samples in a wave");

__device__ __forceinline__ bool dist_row_exists(const AsvEvalDistStats& s, size_t row) {
  const int e = static_cast<int>(row / s.max_robots);
  return static_cast<int>(row - static_cast<size_t>(e) * s.max_robots) < s.n_robots[e];
}

__global__ __launch_bounds__(1024) void eval_dist_scan_kernel(const AsvEvalDistStats s) {
  const size_t NT = static_cast<size_t>(s.n_envs) * s.max_robots;
  const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (row >= NT || !dist_row_exists(s, row)) return;
  const int A = min(max(s.n_act[row], 0), s.n_steps);
  double G = 0.0;
  for (int t = A - 1; t >= 0; --t) {
    const size_t at = static_cast<size_t>(t) * NT + row;
    G = s.reward[at] + s.gamma * G;
    s.g_plane[at] = G;
  }
  s.g0[row] = G;
  s.steps[row] = A;
}

__device__ __forceinline__ double half_butterfly(double v) {   // the sum over the lane's 32-lane half, in every lane
#pragma unroll
  for (int m = kDistS / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

__global__ __launch_bounds__(1024) void eval_dist_stats_kernel(const AsvEvalDistStats s) {
  const size_t NT = static_cast<size_t>(s.n_envs) * s.max_robots;
  const int lane = threadIdx.x & (kWave - 1), j = lane & (kDistS - 1), h = lane / kDistS;
  const size_t row = static_cast<size_t>(blockIdx.x) * (blockDim.x / kWave) + threadIdx.x / kWave;   // wave-uniform
  if (row >= NT || !dist_row_exists(s, row)) return;
  const int A = min(max(s.n_act[row], 0), s.n_steps);
  double pin = 0.0, bias = 0.0, pred0 = 0.0;   // lane 0's are the robot's
  int bin = 0;                                  // lane u: steps with u samples at or below the return
  for (int t0 = 0; t0 < A; t0 += 2) {
    const int t = t0 + h;
    const bool on = t < A;   // the odd half of the last pair of an odd A
    double G = 0.0, z = 0.0, tau = 0.0;
    if (on) {
      const size_t at = static_cast<size_t>(t) * NT + row;
      G = s.g_plane[at];
      z = static_cast<double>(s.z[at * kDistS + j]);
      tau = static_cast<double>(s.tau[at * kDistS + j]);
    }
    const unsigned long long le = __ballot(on && z <= G);
    const int u0 = __popcll(le & 0xFFFFFFFFull), u1 = __popcll(le >> kDistS);
    const double d = G - z;
    const double p = half_butterfly(d * (tau - (d < 0.0 ? 1.0 : 0.0)));
    const double m = half_butterfly(z) * (1.0 / kDistS);
    const double b = m - G;
    const double p1 = __shfl(p, kDistS, kWave), b1 = __shfl(b, kDistS, kWave);
    const bool two = t0 + 1 < A;   // wave-uniform
    if (t0 == 0) pred0 = m;
    pin += p;
    bias += b;
    if (two) {
      pin += p1;
      bias += b1;
    }
    bin += (lane == u0 ? 1 : 0) + (two && lane == u1 ? 1 : 0);
  }
  if (lane < kPitBins) s.pit[row * kPitBins + lane] = bin;
  if (lane == 0) {
    s.pinball[row] = pin;
    s.bias[row] = bias;
    s.pred0[row] = pred0;
  }
}

}  // namespace
}  // namespace asvrl

using namespace asvrl;

extern "C" int64_t asvrl_eval_dist_stats_struct_size(void) { return sizeof(AsvEvalDistStats); }

extern "C" int asvrl_eval_dist_stats(const AsvEvalDistStats* s, void* stream) {
  const std::string who = "asvrl_eval_dist_stats";
  ASVRL_REQUIRE(s != nullptr, who + ": null struct");
  ASVRL_REQUIRE(s->n_steps >= 1, who + ": n_steps must be >= 1");
  ASVRL_REQUIRE(s->n_envs >= 1, who + ": n_envs must be >= 1");
  ASVRL_REQUIRE(s->max_robots >= 1 && s->max_robots <= 32, who + ": max_robots must be in 1..32");
  ASVRL_REQUIRE(s->block == 0 || (s->block >= kWave && s->block <= 1024 && s->block % kWave == 0),
                who + ": block must be 0 or a multiple of 64 up to 1024");
  ASVRL_REQUIRE(s->gamma == s->gamma && s->gamma >= 0.0 && s->gamma <= 1.0, who + ": gamma must be in [0, 1]");
#define ASVRL_DIST_ARRAY(name) ASVRL_REQUIRE(s->name != nullptr, who + ": null array " #name)
  ASVRL_DIST_ARRAY(z);
  ASVRL_DIST_ARRAY(tau);
  ASVRL_DIST_ARRAY(reward);
  ASVRL_DIST_ARRAY(n_act);
  ASVRL_DIST_ARRAY(n_robots);
  ASVRL_DIST_ARRAY(g_plane);
  ASVRL_DIST_ARRAY(g0);
  ASVRL_DIST_ARRAY(pred0);
  ASVRL_DIST_ARRAY(pit);
  ASVRL_DIST_ARRAY(pinball);
  ASVRL_DIST_ARRAY(bias);
  ASVRL_DIST_ARRAY(steps);
#undef ASVRL_DIST_ARRAY
  const int block = s->block == 0 ? 256 : s->block;
  const long long NT = static_cast<long long>(s->n_envs) * s->max_robots;
  hipLaunchKernelGGL(eval_dist_scan_kernel, dim3(static_cast<unsigned>((NT + block - 1) / block)), dim3(block), 0,
                     as_stream(stream), *s);
  if (int rc = check_launch("asvrl_eval_dist_stats (scan)")) return rc;
  const int wpb = block / kWave;
  hipLaunchKernelGGL(eval_dist_stats_kernel, dim3(static_cast<unsigned>((NT + wpb - 1) / wpb)), dim3(block), 0,
                     as_stream(stream), *s);
  return check_launch("asvrl_eval_dist_stats");
}

extern "C" int64_t asvrl_eval_metrics_struct_size(void) { return sizeof(AsvEvalMetrics); }

extern "C" int64_t asvrl_eval_history_struct_size(void) { return sizeof(AsvEvalHistory); }

extern "C" int32_t asvrl_eval_history_step_tile(void) { return kHistSteps; }

static int eval_history_check(const AsvEvalHistory* h, const std::string& who) {
  ASVRL_REQUIRE(h != nullptr, who + ": null struct");
  ASVRL_REQUIRE(h->n_steps >= 1, who + ": n_steps must be >= 1");
  ASVRL_REQUIRE(h->n_envs >= 1, who + ": n_envs must be >= 1");
  ASVRL_REQUIRE(h->max_robots >= 1 && h->max_robots <= 32, who + ": max_robots must be in 1..32");
  return 0;
}

#define ASVRL_HIST_ARRAY(name) ASVRL_REQUIRE(h->name != nullptr, who + ": null array " #name)

extern "C" int asvrl_eval_history_count(const AsvEvalHistory* h, void* stream) {
  const std::string who = "asvrl_eval_history_count";
  if (eval_history_check(h, who)) return 1;
  ASVRL_HIST_ARRAY(info);
  ASVRL_HIST_ARRAY(length);
  ASVRL_HIST_ARRAY(n_robots);
  ASVRL_HIST_ARRAY(counts);
  const long long NT = static_cast<long long>(h->n_envs) * h->max_robots;
  const int blocks = static_cast<int>((NT + 255) / 256);
  hipLaunchKernelGGL(eval_history_count_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), *h);
  return check_launch("asvrl_eval_history_count");
}

extern "C" int asvrl_eval_history_pack(const AsvEvalHistory* h, void* stream) {
  const std::string who = "asvrl_eval_history_pack";
  if (eval_history_check(h, who)) return 1;
  ASVRL_REQUIRE(h->act_steps >= 1, who + ": act_steps must be >= 1");
  ASVRL_REQUIRE(h->traj_rows >= 0 && h->act_rows >= 0 && h->obs_rows >= 0,
                who + ": traj_rows, act_rows and obs_rows must be >= 0");
  ASVRL_HIST_ARRAY(counts);
  ASVRL_HIST_ARRAY(offsets);
  ASVRL_HIST_ARRAY(rs0);
  ASVRL_HIST_ARRAY(rs);
  ASVRL_HIST_ARRAY(actions);
  ASVRL_HIST_ARRAY(obs0);
  ASVRL_HIST_ARRAY(obs);
  ASVRL_HIST_ARRAY(cnt0);
  ASVRL_HIST_ARRAY(obj_cnt);
  ASVRL_REQUIRE(h->traj != nullptr || h->traj_rows == 0, who + ": null array traj");
  ASVRL_REQUIRE(h->act != nullptr || h->act_rows == 0, who + ": null array act");
  ASVRL_REQUIRE(h->obs_out != nullptr || h->obs_rows == 0, who + ": null array obs_out");
  ASVRL_REQUIRE(h->cnt_out != nullptr || h->obs_rows == 0, who + ": null array cnt_out");
  const auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  ASVRL_REQUIRE(aligned(h->obs0) && aligned(h->obs) && aligned(h->obs_out),
                who + ": obs0, obs and obs_out must be 16-byte aligned");
  const long long NT = static_cast<long long>(h->n_envs) * h->max_robots;
  const int bx = static_cast<int>((NT + kHistRows - 1) / kHistRows);
  const int by = (h->n_steps + 1 + kHistSteps - 1) / kHistSteps;
  ASVRL_REQUIRE(by <= 65535, who + ": n_steps is too large for one launch");
  hipLaunchKernelGGL(eval_history_pack_kernel, dim3(bx, by), dim3(256), 0, as_stream(stream), *h);
  return check_launch("asvrl_eval_history_pack");
}

#undef ASVRL_HIST_ARRAY

extern "C" int asvrl_eval_metrics(const AsvEvalMetrics* m, void* stream) {
  const std::string who = "asvrl_eval_metrics";
  ASVRL_REQUIRE(m != nullptr, who + ": null struct");
  ASVRL_REQUIRE(m->n_steps >= 1, who + ": n_steps must be >= 1");
  ASVRL_REQUIRE(m->n_envs >= 1, who + ": n_envs must be >= 1");
  ASVRL_REQUIRE(m->max_robots >= 1 && m->max_robots <= 32, who + ": max_robots must be in 1..32");
#define ASVRL_EVAL_ARRAY(name) ASVRL_REQUIRE(m->name != nullptr, who + ": null array " #name)
  ASVRL_EVAL_ARRAY(reward);
  ASVRL_EVAL_ARRAY(info);
  ASVRL_EVAL_ARRAY(rs);
  ASVRL_EVAL_ARRAY(steps_run);
  ASVRL_EVAL_ARRAY(n_robots);
  ASVRL_EVAL_ARRAY(dt);
  ASVRL_EVAL_ARRAY(N);
  ASVRL_EVAL_ARRAY(pc);
  ASVRL_EVAL_ARRAY(length);
  ASVRL_EVAL_ARRAY(ended);
  ASVRL_EVAL_ARRAY(alive);
  ASVRL_EVAL_ARRAY(deact);
  ASVRL_EVAL_ARRAY(outcome);
  ASVRL_EVAL_ARRAY(ret);
  ASVRL_EVAL_ARRAY(time);
  ASVRL_EVAL_ARRAY(energy);
#undef ASVRL_EVAL_ARRAY
  const int epw = kWave / m->max_robots;
  const int waves = (m->n_envs + epw - 1) / epw;
  const int wpb = 256 / kWave;
  const int blocks = (waves + wpb - 1) / wpb;
  hipLaunchKernelGGL(eval_metrics_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), *m);
  return check_launch("asvrl_eval_metrics");
}
