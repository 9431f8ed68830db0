// asvrl_eval.hip -- the evaluation bookkeeping of Trainer.evaluation (trainer.py:286-303) over the records of
// one hold_done rollout window: asvrl_eval_metrics.
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

}  // namespace
}  // namespace asvrl

using namespace asvrl;

extern "C" int64_t asvrl_eval_metrics_struct_size(void) { return sizeof(AsvEvalMetrics); }

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
