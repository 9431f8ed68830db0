// asvrl_env.hip -- the vectorised ASV marine-env step and reset on gfx950.
//
// Replaces MarineNavEnv3.step / reset (rfarl/rfarl/envs/marinenav/env.py:72-164,240-333)
// and the per-robot Robot methods they call (rfarl/rfarl/envs/marinenav/vehicles/wamv.py).
//
// Layout: robot state is field-major SoA in HBM (rs[field][e * R + i]). A 256-lane workgroup
// owns about 40 robots' worth of whole envs, lane = (env_in_block, robot) in its first wave.
// Phase 1 runs the N Fossen substeps of each robot entirely in registers (f64, one sincos per
// substep). The post-move positions/velocities of the block's robots, their frames and the envs'
// buoys are then staged in LDS; phase 2a gives every (robot, candidate) pair of the block one lane
// across all four waves (noisy observation, detection, collision, sort key into LDS), and phase 2b
// merges each robot's candidates in the reference's order (stable top-5 insertion), then COLREGs,
// reward, done/info and -- in the fused training loop -- trainer.py's deactivation and the
// episode-end test, reduced per env through LDS. (AsvEnvLaunch layout 2: the per-robot sweep, phase 2
// as one serial loop per lane, 64-lane groups.)
//
// Arithmetic follows the reference's operation order (np.matrix products as explicit row
// sums, no FMA contraction: built with -ffp-contract=off) so f64 state agrees with the
// reference to ~1e-14 and collision/goal/done masks bit-exactly.
#include <type_traits>

#include "asvrl_common.h"
#include "asvrl_vonmises_k1.h"
#include "asvrl_actor_tile.h"
#include "asvrl_dqn_tile.h"
#include "asvrl_sac_tile.h"

namespace asvrl {
namespace {

constexpr int kBlock = 256;
// env-step workgroup: one wave of whole envs when they fit (R <= 64), spreading a 4096-env batch
// over every CU instead of packing 51 envs per 256-lane group onto a third of them
__host__ __device__ constexpr int step_block(int R) { return R <= 64 ? 64 : 256; }
// the policy rollout's LDS rows (observations, actions) start at the first 16-byte boundary behind the pair carve
__host__ __device__ constexpr size_t policy_rows_offset(size_t carve_bytes) { return (carve_bytes + 15) & ~size_t{15}; }
constexpr int kMaxCores = 16;        // the device reset sampler's LDS table (env_reset_kernel)
constexpr int kMaxCoresStep = 4096;  // the step and the current field read the cores from HBM

struct Regs {
  double x, y, th, vr0, vr1, vr2, v0, v1, v2, tl, tr, lp, rp;
};

// The pair kernels' arguments, read through the kernarg segment pointer (KArg) rather than as by-value
// parameters: a by-value struct parameter is loaded whole at kernel entry and held to its last use, which
// spilled 122 SGPRs to VGPR lanes (a v_readlane at every later use). A field loaded after kfresh() is not
// merged with the same field's earlier load, so each phase below re-reads what it uses from the kernarg
// segment (scalar loads) and holds it for that phase only.
struct PairsArgs {
  AsvParams p;
  AsvEnvState s;
  AsvStepCtl ctl;
  AsvStepOut out;
  const double* actions;
  const double* noise;
  int epb, group0;
};

__device__ inline double clampd(double v, double lo, double hi) {  // np.clip
  return v < lo ? lo : (v > hi ? hi : v);
}

// env.py:458-501. Cores contribute in ascending-distance order (KDTree query with k = all).
__device__ inline void current_at(const double* __restrict__ cores, int nc, double core_r, double x,
                                  double y, double& cx, double& cy) {
  cx = 0.0;
  cy = 0.0;
  if (nc <= 0) return;
  double prev_d = -1.0;
  int prev_k = -1;
  for (int t = 0; t < nc; ++t) {
    double best_d = 0.0;
    int best_k = -1;
    for (int k = 0; k < nc; ++k) {
      const double dx = cores[4 * k] - x, dy = cores[4 * k + 1] - y;
      const double d = sqrt(dx * dx + dy * dy);
      const bool after = (d > prev_d) || (d == prev_d && k > prev_k);
      if (after && (best_k < 0 || d < best_d)) {
        best_d = d;
        best_k = k;
      }
    }
    prev_d = best_d;
    prev_k = best_k;
    const double* c = cores + 4 * best_k;
    double rx = c[0] - x, ry = c[1] - y;
    const double dis = sqrt(rx * rx + ry * ry);
    rx /= dis;
    ry /= dis;
    double tx, ty;
    if (c[2] != 0.0) { tx = -ry; ty = rx; } else { tx = ry; ty = -rx; }
    const double sp = dis <= core_r ? c[3] / (2 * kPi * core_r * core_r) * dis : c[3] / (2 * kPi * dis);
    cx += tx * sp;
    cy += ty * sp;
  }
}

// One robot's action: N substeps of Robot.update_state (wamv.py:204-231) + compute_motion
// (wamv.py:233-279) with the current sampled at the pre-move position (env.py:257-260).
// The parameters as a plain reference (the sweep kernel) or re-read from the kernarg segment at every substep
// (the pair kernel: the substep loop then holds no parameter in SGPRs across iterations)
struct ParamsRef {
  const AsvParams* q;
  __device__ void fresh() {}
  __device__ const AsvParams& get() const { return *q; }
};
struct ParamsKArg {
  KArg<AsvParams> q;
  __device__ void fresh() { q = kfresh(q); }
  __device__ const AsvParams& get() const { return kref(q); }
};
template <class PR>
__device__ inline void robot_act(PR P, Regs& r, double a0, double a1, int continuous, const double* cores, int nc) {
  // propulsion (wamv.py:251-264) depends only on the thrusts, which change on substep 0
  double fx = 0, fy = 0, mn = 0;
  const double clp = cos(r.lp), slp = sin(r.lp), crp = cos(r.rp), srp = sin(r.rp);
  const int n_sub = P.get().N;
  for (int idx = 0; idx < n_sub; ++idx) {
    P.fresh();
    const AsvParams& p = P.get();
    double cx = 0.0, cy = 0.0;
    if (nc > 0) current_at(cores, nc, p.core_r, r.x, r.y, cx, cy);
    r.v0 = r.vr0 + cx;  // update_velocity (wamv.py:201-202)
    r.v1 = r.vr1 + cy;
    r.v2 = r.vr2 + 0.0;
    r.x += r.v0 * p.dt;
    r.y += r.v1 * p.dt;
    r.th += r.v2 * p.dt;
    while (r.th < 0.0) r.th += kTwoPi;
    while (r.th >= kTwoPi) r.th -= kTwoPi;
    if (idx == 0) {
      double l, rr;
      if (continuous) {
        l = a0 * 1000.0;
        rr = a1 * 1000.0;
      } else {
        const int a = static_cast<int>(a0);
        l = p.left_thrust_change[a / 5];
        rr = p.right_thrust_change[a % 5];
      }
      r.tl = clampd(r.tl + l * p.dt * p.N, p.min_thrust, p.max_thrust);
      r.tr = clampd(r.tr + rr * p.dt * p.N, p.min_thrust, p.max_thrust);
      const double fxl = r.tl * clp, fyl = r.tl * slp;
      const double fxr = r.tr * crp, fyr = r.tr * srp;
      const double mxl = fxl * p.width / 2, myl = -fyl * p.length / 2;
      const double mxr = -fxr * p.width / 2, myr = -fyr * p.length / 2;
      fx = fxl + fxr;
      fy = fyl + fyr;
      mn = mxl + myl + mxr + myr;
    }
    // compute_motion
    double s, c;
    sincos(r.th, &s, &c);
    const double u_r = c * r.vr0 + s * r.vr1;
    const double v_r = -s * r.vr0 + c * r.vr1;
    const double u = c * r.v0 + s * r.v1;
    const double v = -s * r.v0 + c * r.v1;
    const double w = r.v2;
    const double mr = p.m * w;
    const double cv0 = -(-mr * v), cv1 = -(mr * u), cv2 = 0.0;
    const double ca02 = p.yDotV * v_r + p.yDotR * w;
    const double ca12 = -p.xDotU * u_r;
    const double ca20 = -p.yDotV * v_r - p.yDotR * w;
    const double ca21 = p.xDotU * u_r;
    const double au = fabs(u_r), av = fabs(v_r), ar = fabs(w);
    const double n00 = (0.0 + -p.xU) + -(p.xUU * au);
    const double n02 = (ca02 + -0.0) + -0.0;
    const double n11 = (0.0 + -p.yV) + -(p.yVV * av + p.yRV * ar);
    const double n12 = (ca12 + -p.yR) + -(p.yVR * av + p.yRR * ar);
    const double n20 = (ca20 + -0.0) + -0.0;
    const double n21 = (ca21 + -p.nV) + -(p.nVV * av + p.nRV * ar);
    const double n22 = (0.0 + -p.nR) + -(p.nVR * av + p.nRR * ar);
    const double nv0 = n00 * u_r + 0.0 * v_r + n02 * w;
    const double nv1 = 0.0 * u_r + n11 * v_r + n12 * w;
    const double nv2 = n20 * u_r + n21 * v_r + n22 * w;
    const double b0 = cv0 - nv0 + fx, b1 = cv1 - nv1 + fy, b2 = cv2 - nv2 + mn;
    const double acc0 = p.P[0] * b0 + p.P[1] * b1 + p.P[2] * b2;
    const double acc1 = p.P[3] * b0 + p.P[4] * b1 + p.P[5] * b2;
    const double acc2 = p.P[6] * b0 + p.P[7] * b1 + p.P[8] * b2;
    const double w0 = u_r + acc0 * p.dt, w1 = v_r + acc1 * p.dt, w2 = w + acc2 * p.dt;
    r.vr0 = c * w0 + -s * w1;
    r.vr1 = s * w0 + c * w1;
    r.vr2 = w2;
  }
}

__device__ inline double wrap_to_pi(double a) {  // wamv.py:425-434
  while (a < -kPi) a += kTwoPi;
  while (a >= kPi) a -= kTwoPi;
  return a;
}

// reward / done / info (env.py:290-331) and the trainer's bookkeeping (trainer.py:157-172): the
// discounted return gamma^ep_ts * r and deactivation on collision or goal
struct StepResult {
  double reward, ret;
  uint8_t done, info, nfl;
};

__device__ inline StepResult step_result(const AsvParams& p, const AsvStepCtl& ctl, bool exists, bool deact,
                                         bool active, int ep_ts, uint8_t fl, bool coll, bool reach, bool apply,
                                         double phi, double reward, double ret) {
  uint8_t done = 1, info = ASVRL_INFO_ABSENT;
  if (exists) {
    if (deact) {
      reward = 0.0;
      done = 1;
      info = coll ? ASVRL_INFO_DEACT_COLLISION : (reach ? ASVRL_INFO_DEACT_GOAL : ASVRL_INFO_ABSENT);
    } else if (ctl.do_dynamics) {
      double pen = 0.0;
      if (apply) pen += p.COLREGs_penalty * phi;
      reward += pen;
      if (ep_ts >= p.episode_limit) {
        done = 1;
        info = ASVRL_INFO_TOO_LONG;
      } else if (coll) {
        reward += p.collision_penalty;
        done = 1;
        info = ASVRL_INFO_COLLISION;
      } else if (reach) {
        reward += p.goal_reward;
        done = 1;
        info = ASVRL_INFO_REACH_GOAL;
      } else {
        done = 0;
        info = ASVRL_INFO_NORMAL;
      }
    } else {
      done = 0;
      info = ASVRL_INFO_NORMAL;
    }
  }
  uint8_t nfl = static_cast<uint8_t>((fl & ASVRL_FLAG_DEACTIVATED) | (coll ? ASVRL_FLAG_COLLISION : 0) |
                                     (reach ? ASVRL_FLAG_REACH_GOAL : 0) | (apply ? ASVRL_FLAG_COLREGS : 0));
  if (active && ctl.do_dynamics && ctl.trainer_deactivate) {
    if (ctl.gamma > 0) ret += pow(ctl.gamma, static_cast<double>(ep_ts)) * reward;
    if (coll || reach) nfl |= ASVRL_FLAG_DEACTIVATED;
  }
  return StepResult{reward, ret, done, info, nfl};
}

// per-env end of the step (env.py:330, trainer.py:172): episode counter, episode end when the limit is
// hit or no robot is left active, and the finished episode's totals. ret_of(j) / flags_of(j): robot j's
// return and flags after the step (the single step reads them back from HBM, the K-step rollout from LDS)
template <class RetOf, class FlagsOf>
__device__ inline void env_end_from(const AsvParams& p, const AsvEnvState& s, const AsvStepCtl& ctl,
                                    const AsvStepOut& out, int e, int ep_ts, int nrob, int alive, RetOf ret_of,
                                    FlagsOf flags_of) {
  s.ep_ts[e] = ep_ts + 1;
  if (ctl.trainer_deactivate && out.env_done != nullptr) {
    const bool end = (ep_ts >= p.episode_limit) || alive == 0;
    out.env_done[e] = end ? 1 : 0;
    if (end && out.stats != nullptr) {
      double sr = 0, sc = 0, sg = 0, sk = 0, st = 0;
      for (int j = 0; j < nrob; ++j) {
        const uint8_t fj = flags_of(j);
        sr += ret_of(j);
        sc += 1;
        sg += (fj & ASVRL_FLAG_REACH_GOAL) ? 1 : 0;
        sk += (fj & ASVRL_FLAG_COLLISION) ? 1 : 0;
        st += (fj & ASVRL_FLAG_DEACTIVATED) ? 0 : 1;
      }
      atomicAdd(out.stats + 0, sr);
      atomicAdd(out.stats + 1, sc);
      atomicAdd(out.stats + 2, sg);
      atomicAdd(out.stats + 3, sk);
      atomicAdd(out.stats + 4, st);
      atomicAdd(out.stats + 5, 1.0);
    }
  }
}
__device__ inline void env_end(const AsvParams& p, const AsvEnvState& s, const AsvStepCtl& ctl,
                               const AsvStepOut& out, int e, int ep_ts, int nrob, int alive, size_t NT) {
  const size_t e0 = static_cast<size_t>(e) * s.max_robots;
  env_end_from(p, s, ctl, out, e, ep_ts, nrob, alive, [&](int j) { return s.rs[ASVRL_F_RET * NT + e0 + j]; },
               [&](int j) { return s.rflags[e0 + j]; });
}

// check_apply_COLREGs (wamv.py:398-423) for one kept object. `ev` says whether the test got as far as
// the turn angle (the reference assigns phi exactly then); returns phi > 0.
__device__ __forceinline__ bool colregs_body(double rself, double c, double s, double v0, double v1, double ox,
                                             double oy, double ovx, double ovy, double orad, double& phi, bool& ev) {
  ev = false;
  if (sqrt(ovx * ovx + ovy * ovy) < 0.5) return false;
  const double ev0 = c * v0 + s * v1;
  const double ev1 = -s * v0 + c * v1;
  if (sqrt(ev0 * ev0 + ev1 * ev1) < 0.5) return false;
  const double al = atan2(ovy, ovx);  // project_ego_to_vehicle_frame (wamv.py:324-342)
  double sa, ca;
  sincos(al, &sa, &ca);
  const double px = -ca * ox + -sa * oy;
  const double py = sa * ox + -ca * oy;
  const double qx = ca * ev0 + sa * ev1;
  const double qy = -sa * ev0 + ca * ev1;
  const bool x_in = (px >= -9.0) && (px <= 12.0);  // wamv.py:344-362
  const bool y_in = (py >= -17.0) && (py <= 0.0);
  const bool in_tri = (py - (-7.0)) > (-7.0 / 12.0) * (px - 12.0);
  const bool left_pos = x_in && y_in && !in_tri;
  const bool head_pos = (px >= 0.0) && (px <= 17.0) && (py >= -0.5 * 9.0) && (py <= 0.5 * 9.0);  // :364-377
  if (!(left_pos || head_pos)) return false;   // the heading test below cannot rescue either zone
  const double ang = atan2(qy, qx);
  const bool left = left_pos && (ang >= kPi / 4) && (ang <= 3 * kPi / 4);
  const bool head = head_pos && (fabs(ang) > 3 * kPi / 4);
  if (!(left || head)) return false;
  const double ego_ang = atan2(ev1, ev0);  // compute_COLREGs_turn_angle (wamv.py:379-396)
  const double obj_ang = atan2(oy, ox);
  const double base1 = orad + 1.0;
  const double dist = sqrt(ox * ox + oy * oy);
  const double add1 = asin(base1 / dist);
  const double tang = sqrt(dist * dist - base1 * base1);
  const double add2 = atan2(rself, tang);
  const double desired = wrap_to_pi(obj_ang + add1 + add2);
  phi = wrap_to_pi(desired - ego_ang);
  ev = true;
  return phi > 0;
}

// called out of line: its f64 atan2 / asin / sincos inlined at a call site would set the whole kernel's
// register budget (the pair kernel: 162 -> 133 VGPRs)
__device__ __attribute__((noinline)) bool colregs_ev(double rself, double c, double s, double v0, double v1,
                                                     double ox, double oy, double ovx, double ovy, double orad,
                                                     double& phi, bool& ev) {
  return colregs_body(rself, c, s, v0, v1, ox, oy, ovx, ovy, orad, phi, ev);
}

// the per-robot sweep's serial chain (phi written when evaluated)
__device__ __attribute__((noinline)) bool colregs(double rself, double c, double s, double v0, double v1,
                               double ox, double oy, double ovx, double ovy, double orad,
                               double& phi) {
  bool ev;
  return colregs_body(rself, c, s, v0, v1, ox, oy, ovx, ovy, orad, phi, ev);
}

struct Cand {
  double key, a, b, c, d, e;
};

__device__ inline void cswap(bool cond, Cand& x, Cand& y) {
  if (cond) {
    const Cand t = x;
    x = y;
    y = t;
  }
}

// vonmises(0, 1) by its inverse CDF (asvrl_vonmises_k1.h, 1025 f32 knots) at the uniform u, linearly
// interpolated: no rejection loop (Best-Fisher's one or two extra Philox calls per draw, and a wave runs
// the second whenever one of its 64 lanes rejects twice)
__device__ __forceinline__ float vonmises_k1_icdf(float u) {
  const float x = u * static_cast<float>(kVmIcdfN);
  const int i = min(static_cast<int>(x), kVmIcdfN - 1);
  const float lo = kVmIcdfK1[i], hi = kVmIcdfK1[i + 1];
  return lo + (x - static_cast<float>(i)) * (hi - lo);
}

// perception noise of (robot qidx, candidate slot): injected (noise_mode 0, [robot][O + R][5]), f64
// Philox (1) or f32 Philox (2), the substream keyed by (robot, slot) so every launch shape draws the same
// NM: the mode fixed at compile time (the pair kernel's instances), -1: read from ctl. VM = false skips the
// von Mises radius draw n4 (a rejection loop, the costly part; it comes after the four Gaussians in the
// substream, so the Gaussians are the same either way)
template <int NM, bool VM = true>
__device__ __forceinline__ void draw_noise(const AsvParams& p, const AsvStepCtl& ctl, uint64_t ctr,
                                          const double* __restrict__ noise, size_t qidx, int slot, int S,
                                          double& n0, double& n1, double& n2, double& n3, double& n4) {
  const int mode = NM >= 0 ? NM : ctl.noise_mode;
  if (mode == 0) {
    const double* nz = noise + (qidx * static_cast<size_t>(S) + slot) * 5;
    n0 = nz[0]; n1 = nz[1]; n2 = nz[2]; n3 = nz[3];
    if (VM) n4 = nz[4];
  } else if (mode == 1) {
    Stream rng(ctl.seed ^ (ctr >> 32) * 0x9E3779B97F4A7C15ull, static_cast<uint32_t>(qidx),
               (static_cast<uint32_t>(qidx >> 32) ^ 0x5EEDu) + (static_cast<uint32_t>(slot) << 20),
               static_cast<uint32_t>(ctr));
    rng.normal2(n0, n1);
    rng.normal2(n2, n3);
    n0 *= p.pos_std; n1 *= p.pos_std; n2 *= p.vel_std; n3 *= p.vel_std;
    if (VM) n4 = rng.vonmises(p.r_kappa);
  } else {
    StreamF rngf(ctl.seed ^ (ctr >> 32) * 0x9E3779B97F4A7C15ull, static_cast<uint32_t>(qidx),
                 (static_cast<uint32_t>(qidx >> 32) ^ 0xF32Au) + (static_cast<uint32_t>(slot) << 20),
                 static_cast<uint32_t>(ctr));
    float f0, f1, f2, f3, u;
    rngf.normal4u(f0, f1, f2, f3, u);
    n0 = f0 * p.pos_std; n1 = f1 * p.pos_std; n2 = f2 * p.vel_std; n3 = f3 * p.vel_std;
    // the default radius noise (r_kappa = 1, wamv.py:24) from the table; other kappas by rejection
    if (VM) n4 = p.r_kappa == 1.0 ? vonmises_k1_icdf(u) : rngf.vonmises(static_cast<float>(p.r_kappa));
  }
}

// Per-robot sweep (AsvEnvLaunch layout 2): one lane per robot, BLOCK / R whole envs per workgroup;
// perception is one serial loop over the robot's candidates (wamv.py:478-511), top-5 kept in registers.
// PR: every robot's own vehicle / perception parameters from s.robot_params (reset_with_eval_config,
// env.py:553-607); the env-level members (rewards, episode limit, core radius) stay p's.
template <int BLOCK, bool PR>
__global__ __launch_bounds__(BLOCK) void env_sweep_kernel(AsvParams p, AsvEnvState s,
                                                          const double* __restrict__ actions,
                                                          const double* __restrict__ noise,
                                                          AsvStepCtl ctl, AsvStepOut out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = s.max_robots;
  const int O = s.max_obs;
  const int epb = BLOCK / R;
  const int tid = threadIdx.x;
  const int le = tid / R;
  const int i = tid - le * R;
  const int e = blockIdx.x * epb + le;
  const bool lane_env = (le < epb) && (e < s.n_envs);
  const bool env_on = lane_env && (ctl.env_mask == nullptr || ctl.env_mask[e] != 0);
  if (ctl.env_mask != nullptr && !__syncthreads_or(env_on ? 1 : 0)) return;   // no env of the workgroup is on
  const int nrob = lane_env ? s.n_robots[e] : 0;
  const bool exists = env_on && i < nrob;
  const size_t NT = static_cast<size_t>(s.n_envs) * R;
  const size_t idx = static_cast<size_t>(e) * R + i;
  const AsvParams& P = PR ? s.robot_params[exists ? idx : 0] : p;   // this robot's parameters

  // LDS carve: positions/velocities of the block's robots after the move, their pre-step
  // deactivated flags, the envs' obstacles and per-env reductions.
  double* sx = reinterpret_cast<double*>(smem);
  double* sy = sx + BLOCK;
  double* sv0 = sy + BLOCK;
  double* sv1 = sv0 + BLOCK;
  double* sob = sv1 + BLOCK;                 // [epb][O][3]
  int* salive = reinterpret_cast<int*>(sob + static_cast<size_t>(epb) * O * 3);  // [epb]
  unsigned char* soff = reinterpret_cast<unsigned char*>(salive + epb);         // [BLOCK]

  Regs r{};
  uint8_t fl = 0;
  if (exists) {
    const double* rs = s.rs;
    r.x = rs[ASVRL_F_X * NT + idx];
    r.y = rs[ASVRL_F_Y * NT + idx];
    r.th = rs[ASVRL_F_THETA * NT + idx];
    r.vr0 = rs[ASVRL_F_VR0 * NT + idx];
    r.vr1 = rs[ASVRL_F_VR1 * NT + idx];
    r.vr2 = rs[ASVRL_F_VR2 * NT + idx];
    r.v0 = rs[ASVRL_F_V0 * NT + idx];
    r.v1 = rs[ASVRL_F_V1 * NT + idx];
    r.v2 = rs[ASVRL_F_V2 * NT + idx];
    r.tl = rs[ASVRL_F_TL * NT + idx];
    r.tr = rs[ASVRL_F_TR * NT + idx];
    r.lp = rs[ASVRL_F_LP * NT + idx];
    r.rp = rs[ASVRL_F_RP * NT + idx];
    fl = s.rflags[idx];
  }
  const bool deact = (fl & ASVRL_FLAG_DEACTIVATED) != 0;
  const bool active = exists && !deact;
  const int ep_ts = env_on ? s.ep_ts[e] : 0;
  double gx = 0, gy = 0;
  if (exists) {
    gx = s.rs[ASVRL_F_GX * NT + idx];
    gy = s.rs[ASVRL_F_GY * NT + idx];
  }

  // ---------------- phase 1: dynamics (env.py:247-277)
  double reward = 0.0;
  if (active && ctl.do_dynamics) {
    const double d_before = sqrt((gx - r.x) * (gx - r.x) + (gy - r.y) * (gy - r.y));
    const int nc = s.n_cores[e];
    const double* cores = s.cores + static_cast<size_t>(e) * s.max_cores * 4;
    robot_act(ParamsRef{&P}, r, actions[2 * idx], actions[2 * idx + 1], ctl.is_continuous, cores,
              nc < s.max_cores ? nc : s.max_cores);
    const double d_after = sqrt((gx - r.x) * (gx - r.x) + (gy - r.y) * (gy - r.y));
    reward = 0.0;
    reward += p.timestep_penalty;
    reward += d_before - d_after;
  }

  // ---------------- stage for perception
  sx[tid] = r.x;
  sy[tid] = r.y;
  sv0[tid] = r.v0;
  sv1[tid] = r.v1;
  soff[tid] = exists ? (deact ? 1 : 0) : 1;
  if (env_on) {
    const int no = s.n_obs[e];
    for (int k = i; k < O; k += R) {
      const double* ob = s.obstacles + (static_cast<size_t>(e) * O + k) * 3;
      double* dst = sob + (static_cast<size_t>(le) * O + k) * 3;
      if (k < no) {
        dst[0] = ob[0];
        dst[1] = ob[1];
        dst[2] = ob[2];
      }
    }
    if (i == 0) salive[le] = 0;
  }
  __syncthreads();

  // ---------------- phase 2: perception_output (wamv.py:436-529)
  bool coll = (fl & ASVRL_FLAG_COLLISION) != 0;
  bool reach = (fl & ASVRL_FLAG_REACH_GOAL) != 0;
  bool apply = false;
  double phi = exists ? s.rs[ASVRL_F_PHI * NT + idx] : 0.0;
  int cnt = -1;
  Cand t0{INFINITY, 0, 0, 0, 0, 0}, t1 = t0, t2 = t0, t3 = t0, t4 = t0;
  double so0 = 0, so1 = 0, so2 = 0, so3 = 0, so4 = 0;
  if (active) {
    double sn, cs;
    sincos(r.th, &sn, &cs);
    const double tx = -(cs * r.x + sn * r.y);
    const double ty = -(-sn * r.x + cs * r.y);
    so0 = (cs * gx + sn * gy) + tx;
    so1 = (-sn * gx + cs * gy) + ty;
    so2 = cs * r.v0 + sn * r.v1;
    so3 = -sn * r.v0 + cs * r.v1;
    so4 = r.v2;
    if (sqrt((gx - r.x) * (gx - r.x) + (gy - r.y) * (gy - r.y)) <= P.goal_dis) reach = true;

    int nkept = 0;
    const int no = s.n_obs[e];
    const int base = le * R;
    const uint64_t ctr = ctl.counter + (ctl.counter_dev != nullptr ? *ctl.counter_dev : 0ull);
    const int ncand = no + nrob;
    const bool full_circle = 0.5 * P.angle >= kPi;
    for (int k = 0; k < ncand; ++k) {
      double ox, oy, orad, vx0, vy0;
      int slot;
      if (k < no) {
        const double* ob = sob + (static_cast<size_t>(le) * O + k) * 3;
        ox = ob[0];
        oy = ob[1];
        orad = ob[2];
        vx0 = 0.0;
        vy0 = 0.0;
        slot = k;
      } else {
        const int j = k - no;
        if (j == i || soff[base + j]) continue;  // self / deactivated (wamv.py:487-491)
        ox = sx[base + j];
        oy = sy[base + j];
        orad = PR ? s.robot_params[static_cast<size_t>(e) * R + j].r : p.r;   // the other robot's r
        vx0 = sv0[base + j];
        vy0 = sv1[base + j];
        slot = O + j;
      }
      double n0, n1, n2, n3, n4;
      draw_noise<-1>(P, ctl, ctr, noise, idx, slot, O + R, n0, n1, n2, n3, n4);
      const double pxn = ox + n0, pyn = oy + n1;  // Perception (wamv.py:27-40)
      const double vxn = vx0 + n2, vyn = vy0 + n3;
      const double rn = P.r_mean_ratio * orad + (1 - P.r_mean_ratio) * n4 / kPi * orad;
      const double qx = (cs * pxn + sn * pyn) + tx, qy = (-sn * pxn + cs * pyn) + ty;
      const double qn = sqrt(qx * qx + qy * qy);
      if (qn > P.range + rn) continue;  // check_detection (wamv.py:293-303)
      if (!full_circle) {              // atan2 lies in [-pi, pi]: the test only bites when angle < 2 pi
        const double ang = atan2(qy, qx);
        if (ang < -0.5 * P.angle || ang > 0.5 * P.angle) continue;
      }
      if (!coll) {  // check_collision (wamv.py:281-291), true positions
        const double d = sqrt((r.x - ox) * (r.x - ox) + (r.y - oy) * (r.y - oy)) - orad - P.r;
        if (d <= 0.0) coll = true;
      }
      Cand cd{qn - rn - P.r, qx, qy, cs * vxn + sn * vyn, -sn * vxn + cs * vyn, rn};
      // heapq.nsmallest == stable ascending order: a new candidate passes equal keys
      cswap(cd.key < t0.key, cd, t0);
      cswap(cd.key < t1.key, cd, t1);
      cswap(cd.key < t2.key, cd, t2);
      cswap(cd.key < t3.key, cd, t3);
      cswap(cd.key < t4.key, cd, t4);
      ++nkept;
    }
    cnt = nkept < P.max_obj_num ? nkept : P.max_obj_num;
    // COLREGs over the kept objects in order, stop at the first hit (wamv.py:517-521)
    if (cnt > 0) apply = colregs(P.r, cs, sn, r.v0, r.v1, t0.a, t0.b, t0.c, t0.d, t0.e, phi);
    if (!apply && cnt > 1) apply = colregs(P.r, cs, sn, r.v0, r.v1, t1.a, t1.b, t1.c, t1.d, t1.e, phi);
    if (!apply && cnt > 2) apply = colregs(P.r, cs, sn, r.v0, r.v1, t2.a, t2.b, t2.c, t2.d, t2.e, phi);
    if (!apply && cnt > 3) apply = colregs(P.r, cs, sn, r.v0, r.v1, t3.a, t3.b, t3.c, t3.d, t3.e, phi);
    if (!apply && cnt > 4) apply = colregs(P.r, cs, sn, r.v0, r.v1, t4.a, t4.b, t4.c, t4.d, t4.e, phi);
  }

  const StepResult res = step_result(p, ctl, exists, deact, active, ep_ts, fl, coll, reach, apply, phi, reward,
                                     exists ? s.rs[ASVRL_F_RET * NT + idx] : 0.0);
  if (ctl.trainer_deactivate && ctl.do_dynamics && exists && !(res.nfl & ASVRL_FLAG_DEACTIVATED))
    atomicAdd(&salive[le], 1);

  // ---------------- write back
  if (exists) {
    double* rs = s.rs;
    if (ctl.do_dynamics) {
      rs[ASVRL_F_X * NT + idx] = r.x;
      rs[ASVRL_F_Y * NT + idx] = r.y;
      rs[ASVRL_F_THETA * NT + idx] = r.th;
      rs[ASVRL_F_VR0 * NT + idx] = r.vr0;
      rs[ASVRL_F_VR1 * NT + idx] = r.vr1;
      rs[ASVRL_F_VR2 * NT + idx] = r.vr2;
      rs[ASVRL_F_V0 * NT + idx] = r.v0;
      rs[ASVRL_F_V1 * NT + idx] = r.v1;
      rs[ASVRL_F_V2 * NT + idx] = r.v2;
      rs[ASVRL_F_TL * NT + idx] = r.tl;
      rs[ASVRL_F_TR * NT + idx] = r.tr;
      rs[ASVRL_F_RET * NT + idx] = res.ret;
    }
    rs[ASVRL_F_PHI * NT + idx] = phi;
    s.rflags[idx] = res.nfl;
  }
  if (env_on && i < R) {
    // packed f32 obs row (replay_buffer.py:51-69 + the .float() of agent.py:363-366)
    float4* o4 = reinterpret_cast<float4*>(out.obs + idx * ASVRL_OBS_DIM);
    const bool a = active;
    const float m0 = (a && cnt > 0) ? 1.f : 0.f, m1 = (a && cnt > 1) ? 1.f : 0.f,
                m2 = (a && cnt > 2) ? 1.f : 0.f, m3 = (a && cnt > 3) ? 1.f : 0.f,
                m4 = (a && cnt > 4) ? 1.f : 0.f;
    auto f = [](double v, float m) { return m != 0.f ? static_cast<float>(v) : 0.f; };
    const float sf = a ? 1.f : 0.f;
    o4[0] = make_float4(f(so0, sf), f(so1, sf), f(so2, sf), f(so3, sf));
    o4[1] = make_float4(f(so4, sf), f(r.tl, sf), f(r.tr, sf), f(t0.a, m0));
    o4[2] = make_float4(f(t0.b, m0), f(t0.c, m0), f(t0.d, m0), f(t0.e, m0));
    o4[3] = make_float4(f(t1.a, m1), f(t1.b, m1), f(t1.c, m1), f(t1.d, m1));
    o4[4] = make_float4(f(t1.e, m1), f(t2.a, m2), f(t2.b, m2), f(t2.c, m2));
    o4[5] = make_float4(f(t2.d, m2), f(t2.e, m2), f(t3.a, m3), f(t3.b, m3));
    o4[6] = make_float4(f(t3.c, m3), f(t3.d, m3), f(t3.e, m3), f(t4.a, m4));
    o4[7] = make_float4(f(t4.b, m4), f(t4.c, m4), f(t4.d, m4), f(t4.e, m4));
    o4[8] = make_float4(m0, m1, m2, m3);
    o4[9] = make_float4(m4, 0.f, 0.f, 0.f);
    if (out.obs64 != nullptr) {
      double* o = out.obs64 + idx * 32;
      const double v[32] = {so0, so1, so2, so3, so4, r.tl, r.tr,
                            t0.a, t0.b, t0.c, t0.d, t0.e, t1.a, t1.b, t1.c, t1.d, t1.e,
                            t2.a, t2.b, t2.c, t2.d, t2.e, t3.a, t3.b, t3.c, t3.d, t3.e,
                            t4.a, t4.b, t4.c, t4.d, t4.e};
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const bool keep = a && (k < 7 || (k - 7) / 5 < cnt);
        o[k] = keep ? v[k] : 0.0;
      }
    }
    out.obj_cnt[idx] = static_cast<int8_t>(exists ? cnt : -1);
    out.reward[idx] = res.reward;
    out.done[idx] = res.done;
    out.info[idx] = res.info;
  }
  __syncthreads();
  if (env_on && i == 0 && ctl.do_dynamics) env_end(p, s, ctl, out, e, ep_ts, nrob, salive[le], NT);
}

// Pair-parallel env step (AsvEnvLaunch layout 1). A workgroup owns `epb` whole envs; their robots
// occupy its first nrb = epb * R lanes. Phases, each over all lanes, separated by workgroup barriers:
//   1  robot lanes: N Fossen substeps in registers, state written back, the observation's self part,
//      the robot's frame, position and velocity into LDS
//   2  one lane per (robot, candidate slot) pair: noise, detection, collision, sort key -- 13 B per
//      pair in LDS (key, von Mises draw, flag; 17 B with f64 draws)
//   3  robot lanes: the stable top-5 of the keys in the reference's order (slot indices only), collision
//      as an OR
//   4  one lane per kept object (a work list built by a scan of the counts): the object's row
//      recomputed from the same noise draw and arithmetic as in phase 2 (bit-identical; the von Mises
//      radius draw kept from phase 2, the Gaussians redrawn), written into the observation; its
//      COLREGs test
//   5  robot lanes: the first COLREGs hit in order and the phi the reference's serial chain leaves,
//      reward / done / info, trainer bookkeeping; then the per-env episode end
// No phase keeps another's values in registers and LDS holds ~15 KB per 12-env workgroup, so several
// workgroups share a CU (the round-1 form kept 40-B rows per pair and the top-5 rows in registers:
// 239 VGPRs, 35 KB, two waves per SIMD).
#ifndef ASVRL_ENV_PAIRS_WPE
#define ASVRL_ENV_PAIRS_WPE 4
#endif
// the device reset sampler (below, "reset"), which the auto-resetting rollout calls from its step loop
constexpr int kResetWaves = 4;
constexpr int kResetMaxR = 32;
constexpr int kResetMaxO = 32;
// The accepted sets of one env's reset, in the resetting wave's LDS
struct ResetLds {
  double rob[4][kResetMaxR];      // x, y, gx, gy of accepted robots
  double core[kMaxCores][4];      // x, y, clockwise, Gamma
  double obs[kResetMaxO][3];      // x, y, r
};
__device__ __forceinline__ void reset_env(const AsvParams& p, const AsvEnvState& s, const AsvResetCfg& cfg, int e,
                                          uint64_t seed, uint64_t ctr, int lane, ResetLds& W);
// the auto-resetting rollout's LDS behind the carve (and the policy rows): a ResetLds per wave, a flag per env
__host__ __device__ constexpr size_t autoreset_lds(int blk, int epb) {
  return static_cast<size_t>(blk / 64) * sizeof(ResetLds) + sizeof(int) * static_cast<size_t>(epb);
}
// one workgroup's envs [bid * epb, (bid + 1) * epb) of the step (env_pairs_kernel loops over them)
// ROLL (env_rollout_kernel): RO->n_steps open-loop steps in one launch. The robot lanes load their state, goal,
// flags, return, phi and the env's step count once and keep them in registers over the steps; the buoys are
// staged once; step t takes row t of A->actions (and of A->noise in mode 0) and draws at counter + t. The state
// goes back to HBM after the env's last step; every step's outputs go to row t of the kept records, the last
// step's to A->out. The phases are the single step's own code: without ROLL the loop below runs once.
// POL (env_policy_rollout_kernel, with ROLL): closed loop. The AC-IQN Actor (asvrl_actor_tile.h, its weights
// staged once into AL) runs in front of phase 1 of every step on the workgroup's nrb robot rows, wave w on the
// 32-row tiles w, w + waves, ...; it reads the rows of an LDS copy of the observation (PI->obs_in before step 0,
// then what the phases of the step before wrote: they write it beside their global outputs) and leaves the f64
// action pairs in LDS, where phase 1 takes the lane's action instead of from A->actions.
// POL = kPolDqn (the same kernel template): the same closed loop under DQN_Policy -- the Actor's trunk staged the same
// way, the 25-wide head's fragments and bias read from L2 (asvrl_dqn_tile.h: dqn_act_kernel's functions), the first
// arg-max and the epsilon-greedy index left as the pair (index, 0.0), which phase 1 takes as a discrete action.
// POL = kPolSac (likewise): the closed loop under SAC's sampled actor -- the trunk staged the same way,
// the f32 head (2 KB) staged beside it in HL before the staging's barrier, then sac_act_kernel's statements
// (asvrl_sac_tile.h): the two normals of (global row, step) in the act stream, or none when PI->deterministic, the
// head without its log-probability, and atile::explore into the f64 action pair.
// AR (the _ar calls, with ROLL): episodes restart inside the window. After the
// phases of step t the workgroup votes on "an env of mine ended in this step"; if so its waves reset the ended envs
// (reset_env, one wave per env, the waves taking them in turn, each in its own ResetLds behind the carve and the
// policy rows), the robot lanes of those envs reload what the rollout keeps over the steps (state, goal, phi, ret,
// flags, ep_ts, n_robots and with it `exists`, the staged buoys and counts), and the step's own phases run once
// more as the masked observation pass (obsp: no act, no dynamics, no bookkeeping, the draws at obs_counter + t),
// writing A->out, the policy's LDS rows and row t + 1 of the obs_prev record -- never row t of the step's records.
// The second pass is a jump back to the top of the phases, not a loop around them, so the instantiations without AR
// keep their control flow (and their code: compared instruction for instruction). Barriers: the vote, the barriers
// around the reset and the phases' own are reached by every lane of the workgroup: the vote's result is
// workgroup-uniform, the reset loop's trip count depends on the wave index and epb only and its condition (an LDS
// flag per env, through readfirstlane) is wave-uniform, reset_env has wave barriers only, the reload is plain
// lane-predicated code in front of the observation pass's first barrier, and that pass runs the same barrier
// sequence as the step (the act and the env-end sections, which it skips, are skipped by all lanes alike). No lane
// leaves the step loop early (hold_done is refused with AR), and since every lane of an env reads the env's alive
// count for `end`, the vote is also the barrier between those reads and the next step's reset of the count.
// the policy in front of every step of a closed-loop rollout, and its argument struct
enum : int { kPolNone = 0, kPolActor = 1, kPolDqn = 2, kPolSac = 3 };
template <int POL> struct PolicyOf { using type = AsvPolicy; };
template <> struct PolicyOf<kPolDqn> { using type = AsvDqnPolicy; };
template <> struct PolicyOf<kPolSac> { using type = AsvSacPolicy; };
__device__ __forceinline__ const AsvMlpWeights& trunk_of(const AsvPolicy& p) { return p.w; }
__device__ __forceinline__ const AsvMlpWeights& trunk_of(const AsvDqnPolicy& p) { return p.w.trunk; }
__device__ __forceinline__ const AsvMlpWeights& trunk_of(const AsvSacPolicy& p) { return p.w.trunk; }
template <int BLOCK, int NM, bool DYN = true, bool ROLL = false, int POL = kPolNone, bool AR = false>   // DYN false: an observation pass only (do_dynamics = 0)
__device__ __forceinline__ void env_pairs_block(KArg<PairsArgs> A, int epb, int bid, unsigned char* smem,
                                                KArg<AsvRollout> RO = nullptr,
                                                KArg<typename PolicyOf<POL>::type> PI = nullptr,
                                                atile::ActorLds* AL = nullptr, KArg<AsvAutoReset> RS = nullptr,
                                                unsigned char* ar_lds = nullptr,
                                                sactile::SacHeadLds* HL = nullptr) {
  static_assert(POL == kPolNone || ROLL, "the policy runs inside the rollout's step loop");
  static_assert(!AR || ROLL, "the auto-reset runs inside the rollout's step loop");
  const int R = A->s.max_robots;
  const int O = A->s.max_obs;
  const int S = O + R;               // candidate slots per robot (obstacles, then robots)
  const int nrb = epb * R;
  const int npairs = nrb * S;
  const int nslot = npairs > 5 * nrb ? npairs : 5 * nrb;
  int tid = threadIdx.x;

  double* sx = reinterpret_cast<double*>(smem);   // [nrb] robots after the move
  double* sy = sx + nrb;
  double* sv0 = sy + nrb;
  double* sv1 = sv0 + nrb;
  double* scs = sv1 + nrb;           // robot frame: cos, sin, translation
  double* ssn = scs + nrb;
  double* stx = ssn + nrb;
  double* sty = stx + nrb;
  double* pk = sty + nrb;            // [nslot] phase 2 sort keys; phase 4 phi of (robot, k)
  double* sob = pk + nslot;          // [epb][O][3]
  using VmT = typename std::conditional<NM == 2, float, double>::type;   // the f32 stream's draw is a float
  VmT* pvm = reinterpret_cast<VmT*>(sob + static_cast<size_t>(epb) * O * 3);  // [npairs] von Mises radius draws
  int* salive = reinterpret_cast<int*>(pvm + npairs);  // [epb]
  int* sno = salive + epb;           // [epb] obstacles, robots of each env
  int* snr = sno + epb;
  int* swt = snr + epb;              // [BLOCK / 64] kept objects per wave (phase 3 scan)
  unsigned short* skept = reinterpret_cast<unsigned short*>(swt + BLOCK / kWave);  // [nrb][5] kept slots in order
  unsigned short* sitem = skept + 5 * nrb;   // [5 * nrb] phase 4 work list: robot * 5 + k of every kept object
  unsigned char* pfl = reinterpret_cast<unsigned char*>(sitem + 5 * nrb);  // [nslot] 1 detected | 2 collision; phase 4: 1 evaluated | 2 hit
  unsigned char* soff = pfl + nslot;   // [nrb] not a candidate (absent / deactivated before the step)
  unsigned char* sact = soff + nrb;    // [nrb] active
  signed char* scnt = reinterpret_cast<signed char*>(sact + nrb);  // [nrb] kept count, -1 inactive
  // POL: the robots' observation rows [nrb][ASVRL_OBS_DIM] f32 and action pairs [nrb][2] f64, 16-byte aligned
  float* sobs = reinterpret_cast<float*>(smem + policy_rows_offset(reinterpret_cast<unsigned char*>(scnt + nrb) - smem));
  double* sa64 = reinterpret_cast<double*>(sobs + static_cast<size_t>(nrb) * ASVRL_OBS_DIM);
  const size_t row0 = POL != kPolNone ? static_cast<size_t>(bid) * nrb : 0;   // the workgroup's first global robot row

  const bool rlane = tid < nrb;
  int le = tid / R;
  const int i = tid - le * R;
  const int e = bid * epb + le;
  const bool lane_env = rlane && e < A->s.n_envs;
  const bool env_on0 = lane_env && (A->ctl.env_mask == nullptr || A->ctl.env_mask[e] != 0);
  // a masked pass (the observation pass after a reset) touches few envs: workgroups with none leave
  if (A->ctl.env_mask != nullptr && !__syncthreads_or(env_on0 ? 1 : 0)) return;
  int nrob = lane_env ? A->s.n_robots[e] : 0;   // (AR: reloaded after the env's reset, which may place fewer robots)
  bool exists0 = env_on0 && i < nrob;
  const size_t NT = static_cast<size_t>(A->s.n_envs) * R;
  size_t idx = static_cast<size_t>(e) * R + i;
  // what a rollout keeps over its steps (a single step: this step's values)
  uint8_t flv = exists0 ? A->s.rflags[idx] : 0;
  int ep_ts = env_on0 ? A->s.ep_ts[e] : 0;
  Regs r{};
  double gx = 0, gy = 0, phi = 0.0, ret = 0.0;
  bool on = env_on0;   // hold_done: cleared after the env's end step
  int taken = 0;       // steps the env took
  int nreset = 0;      // AR: resets of the env
  bool rstl = false;   // AR: the lane's env was reset after this step's phases (the lanes of the observation pass)
  const int n_steps = ROLL ? RO->n_steps : 1;
  const bool hold = ROLL && RO->hold_done != 0;
  auto load_state = [&] {
    const double* rs = A->s.rs;
    r.x = rs[ASVRL_F_X * NT + idx];
    r.y = rs[ASVRL_F_Y * NT + idx];
    r.th = rs[ASVRL_F_THETA * NT + idx];
    r.vr0 = rs[ASVRL_F_VR0 * NT + idx];
    r.vr1 = rs[ASVRL_F_VR1 * NT + idx];
    r.vr2 = rs[ASVRL_F_VR2 * NT + idx];
    r.v0 = rs[ASVRL_F_V0 * NT + idx];
    r.v1 = rs[ASVRL_F_V1 * NT + idx];
    r.v2 = rs[ASVRL_F_V2 * NT + idx];
    r.tl = rs[ASVRL_F_TL * NT + idx];
    r.tr = rs[ASVRL_F_TR * NT + idx];
    r.lp = rs[ASVRL_F_LP * NT + idx];
    r.rp = rs[ASVRL_F_RP * NT + idx];
    gx = rs[ASVRL_F_GX * NT + idx];
    gy = rs[ASVRL_F_GY * NT + idx];
  };
  auto store_state = [&] {   // what the dynamics change
    double* rs = A->s.rs;
    rs[ASVRL_F_X * NT + idx] = r.x;
    rs[ASVRL_F_Y * NT + idx] = r.y;
    rs[ASVRL_F_THETA * NT + idx] = r.th;
    rs[ASVRL_F_VR0 * NT + idx] = r.vr0;
    rs[ASVRL_F_VR1 * NT + idx] = r.vr1;
    rs[ASVRL_F_VR2 * NT + idx] = r.vr2;
    rs[ASVRL_F_V0 * NT + idx] = r.v0;
    rs[ASVRL_F_V1 * NT + idx] = r.v1;
    rs[ASVRL_F_V2 * NT + idx] = r.v2;
    rs[ASVRL_F_TL * NT + idx] = r.tl;
    rs[ASVRL_F_TR * NT + idx] = r.tr;
  };
  if constexpr (ROLL) {
    if (exists0) {
      load_state();
      phi = A->s.rs[ASVRL_F_PHI * NT + idx];
      ret = A->s.rs[ASVRL_F_RET * NT + idx];
    }
  }
  if constexpr (POL != kPolNone) {
    // the weights once per workgroup; the rows step 0 acts on (rows past the batch: zeros, never consumed)
    atile::stage_actor<BLOCK>(*AL, trunk_of(kref(PI)), tid);
    if constexpr (POL == kPolSac) sactile::stage_head<BLOCK>(*HL, kref(PI).w, tid);   // (the barrier below is its too)
    constexpr int kRowV = ASVRL_OBS_DIM / 4;
    const float4* src = reinterpret_cast<const float4*>(PI->obs_in);
    for (int k = tid; k < nrb * kRowV; k += BLOCK) {
      const size_t g = row0 + k / kRowV;
      reinterpret_cast<float4*>(sobs)[k] = g < NT ? src[g * kRowV + k % kRowV] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
  }
  if constexpr (AR) {   // row 0 of the acted-on observations: the caller's rows in front of step 0
    const KArg<AsvAutoReset> Q = kfresh(RS);
    const float* src0 = POL != kPolNone ? PI->obs_in : Q->obs_in;
    if (env_on0 && Q->obs_prev != nullptr) {
      const float4* src = reinterpret_cast<const float4*>(src0 + idx * ASVRL_OBS_DIM);
      float4* dst = reinterpret_cast<float4*>(Q->obs_prev + idx * ASVRL_OBS_DIM);
#pragma unroll
      for (int k = 0; k < ASVRL_OBS_DIM / 4; ++k) dst[k] = src[k];
    }
  }

  // the step loop (its body keeps the single step's indentation; closed at "step t" below)
  for (int t = 0; t < n_steps; ++t) {
  if constexpr (ROLL) {
    // the lane's indices, opaque per step: the addresses built on them (17 state fields, records, outputs, LDS
    // rows) are then computed where they are used, as in the single step, not hoisted out of the step loop and
    // held in registers over all of it
    asm volatile("" : "+v"(tid), "+v"(le), "+v"(idx));
    // every env of the workgroup is held: nothing left to do
    if (hold && !__syncthreads_or(on ? 1 : 0)) break;
  }
  // AR: the phases run as the step and then, only behind a reset in this workgroup, once more as the reset envs'
  // observation pass (obsp; the jump back to `phases` is at the end of the step, its only writer)
  bool obsp = false;
  [[maybe_unused]] phases:
  if constexpr (AR) asm volatile("" : "+v"(tid), "+v"(le), "+v"(idx));   // (opaque per pass as per step)
  const bool env_on = ROLL ? (on && (!obsp || rstl)) : env_on0;
  const bool exists = ROLL ? (exists0 && env_on) : exists0;
  const uint8_t fl = flv;
  const bool deact = (fl & ASVRL_FLAG_DEACTIVATED) != 0;
  const bool active = exists && !deact;
  bool coll = (fl & ASVRL_FLAG_COLLISION) != 0;
  bool reach = (fl & ASVRL_FLAG_REACH_GOAL) != 0;
  double reward = 0.0;
  // the step's outputs: A->out (a single step; a rollout's last step, and every step of a held rollout, whose
  // envs end on different steps) and row t of the rollout's kept records, whose members may be null
  const bool wlast = !ROLL || hold || t == n_steps - 1;
  auto rec_row = [&] {
    AsvStepOut o{};
    if constexpr (ROLL) {
      const KArg<AsvRollout> Q = kfresh(RO);   // read where used, not held over the step
      const size_t t0 = static_cast<size_t>(t) * NT;
      o.obs = Q->obs != nullptr ? Q->obs + t0 * ASVRL_OBS_DIM : nullptr;
      o.obj_cnt = Q->obj_cnt != nullptr ? Q->obj_cnt + t0 : nullptr;
      o.reward = Q->reward != nullptr ? Q->reward + t0 : nullptr;
      o.done = Q->done != nullptr ? Q->done + t0 : nullptr;
      o.info = Q->info != nullptr ? Q->info + t0 : nullptr;
    }
    return o;
  };
  // f(o, opt, base): the outputs o (opt: members may be null); o.obs's rows are numbered from global row `base`
  auto each_out = [&](KArg<PairsArgs> Ak, auto&& f) {
    if (wlast) f(kref(Ak).out, std::false_type{}, size_t{0});
    if constexpr (AR) {   // the records of row t keep the step's values, not the reset pass's
      if (!obsp) f(rec_row(), std::true_type{}, size_t{0});
    } else if constexpr (ROLL) {
      f(rec_row(), std::true_type{}, size_t{0});
    }
    if constexpr (POL != kPolNone) {   // the rows the Actor reads at the next step
      AsvStepOut o{};
      o.obs = sobs;
      f(o, std::true_type{}, row0);
    }
    if constexpr (AR) {   // the acted-on observation of step t + 1: what this step, or the reset pass behind it, leaves
      const KArg<AsvAutoReset> Q = kfresh(RS);
      AsvStepOut o{};
      if (Q->obs_prev != nullptr && t + 1 < n_steps)
        o.obs = Q->obs_prev + static_cast<size_t>(t + 1) * NT * ASVRL_OBS_DIM;
      f(o, std::true_type{}, size_t{0});
    }
  };

  // ---------------- act: the Actor on the workgroup's rows, epsilon-greedy at step *step_dev + t
  if constexpr (AR) {
    if (obsp) goto acted;   // (workgroup-uniform) the observation pass acts on nothing
  }
  if constexpr (POL == kPolActor) {
    const KArg<AsvPolicy> P = kfresh(PI);
    const uint64_t step = (P->step_dev != nullptr ? static_cast<uint64_t>(*P->step_dev) : 0ull) + static_cast<uint64_t>(t);
    const int ln = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    for (int tile = wv; tile * 32 < nrb; tile += BLOCK / kWave) {   // wave-uniform: the MFMAs run with every lane on
      // the tile's LDS reads stay inside the loop: its only stores are the f64 action pairs, so the f32 bias and
      // output-layer reads (384 values per lane) would otherwise be hoisted in front of it and spilled
      asm volatile("" ::: "memory");
      const int lr = tile * 32 + (ln & 31);
      const bool valid = lr < nrb;
      frag8 bx[2];
      float mk[atile::kObjN];
      atile::load_obs(sobs, ASVRL_OBS_DIM, valid ? lr : nrb - 1, ln >> 5, bx, mk);
      float z0, z1, a0, a1;
      atile::actor_chain<atile::MLP_ACT>(kref(P).w, AsvMlpIO{}, *AL, 0, false, ln, bx, mk, z0, z1, a0, a1);
      if (valid && ln < 32)
        atile::explore(step, atile::EpsSchedule{P->eps_steps_per_count, P->eps_total, P->eps_fraction, P->eps_initial,
                                                P->eps_final},
                       P->seed, static_cast<int>(row0 + lr), a0, a1, sa64[2 * lr], sa64[2 * lr + 1]);
    }
    __syncthreads();
    if (env_on && P->actions != nullptr) {   // the action every robot slot of a stepping env was given
      double* rec = P->actions + (static_cast<size_t>(t) * NT + idx) * 2;
      rec[0] = sa64[2 * tid];
      rec[1] = sa64[2 * tid + 1];
    }
  } else if constexpr (POL == kPolDqn) {
    // DQN_Policy on the workgroup's rows: dqn_act_kernel's Q tile, arg-max and draw (asvrl_dqn_tile.h)
    const KArg<AsvDqnPolicy> P = kfresh(PI);
    const uint64_t step = (P->step_dev != nullptr ? static_cast<uint64_t>(*P->step_dev) : 0ull) + static_cast<uint64_t>(t);
    const int ln = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    for (int tile = wv; tile * 32 < nrb; tile += BLOCK / kWave) {   // wave-uniform: the MFMAs run with every lane on
      asm volatile("" ::: "memory");   // (the tile's LDS reads stay inside the loop, as the Actor's)
      const int lr = tile * 32 + (ln & 31);
      const bool valid = lr < nrb;
      frag8 bx[2];
      float mk[atile::kObjN];
      atile::load_obs(sobs, ASVRL_OBS_DIM, valid ? lr : nrb - 1, ln >> 5, bx, mk);
      float q[16];
      dqtile::dqn_q_tile<atile::MLP_ACT>(kref(P).w, AsvMlpIO{}, *AL, 0, false, ln, bx, mk, q);
      float best;
      int bi;
      const int nact = P->w.n_actions;
      dqtile::dqn_argmax(q, ln >> 5, nact, best, bi);   // (every lane of the wave is live at its shuffle)
      if (valid && ln < 32) {
        const int act = dqtile::dqn_explore(step, atile::EpsSchedule{P->eps_steps_per_count, P->eps_total, P->eps_fraction,
                                                                     P->eps_initial, P->eps_final},
                                            P->seed, static_cast<int>(row0 + lr), bi, nact);
        sa64[2 * lr] = static_cast<double>(act);
        sa64[2 * lr + 1] = 0.0;
      }
    }
    __syncthreads();
    if (env_on && P->actions != nullptr) {   // the action every robot slot of a stepping env was given
      double* rec = P->actions + (static_cast<size_t>(t) * NT + idx) * 2;
      rec[0] = sa64[2 * tid];
      rec[1] = sa64[2 * tid + 1];
    }
  } else if constexpr (POL == kPolSac) {
    // SAC's actor on the workgroup's rows: sac_act_kernel's trunk, noise, head and draw (asvrl_sac_tile.h)
    const KArg<AsvSacPolicy> P = kfresh(PI);
    const uint64_t step = (P->step_dev != nullptr ? static_cast<uint64_t>(*P->step_dev) : 0ull) + static_cast<uint64_t>(t);
    const int ln = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    for (int tile = wv; tile * 32 < nrb; tile += BLOCK / kWave) {   // wave-uniform: the MFMAs run with every lane on
      asm volatile("" ::: "memory");   // (the tile's LDS reads stay inside the loop, as the Actor's)
      const int lr = tile * 32 + (ln & 31);
      const bool valid = lr < nrb;
      const int rr = valid ? lr : nrb - 1;
      // the draw in front of the trunk, where two floats ride through it: behind it (sac_act_kernel's order; the
      // values do not depend on it) Philox and Box-Muller run with h2 live and the kernel spills three times as much
      float eps[atile::kNa] = {0.f, 0.f};   // deterministic: z = mu, nothing drawn (workgroup-uniform)
      if (P->deterministic == 0)
        sactile::sac_eps(sactile::kSacActStream, static_cast<int>(row0 + rr), step, P->seed, eps[0], eps[1]);
      frag8 bx[2];
      float mk[atile::kObjN];
      atile::load_obs(sobs, ASVRL_OBS_DIM, rr, ln >> 5, bx, mk);
      float h2v[8][8];
      atile::trunk_chain<atile::MLP_ACT>(kref(P).w.trunk, AsvMlpIO{}, *AL, 0, false, ln, bx, mk, h2v);
      sactile::SacSample o;
      sactile::sac_head<false>(*HL, P->w.trunk.out_scale, h2v, ln, eps, o);   // (every lane of the wave is live at its shuffle)
      if (valid && ln < 32)
        atile::explore(step, atile::EpsSchedule{P->eps_steps_per_count, P->eps_total, P->eps_fraction, P->eps_initial,
                                                P->eps_final},
                       P->seed, static_cast<int>(row0 + lr), o.a[0], o.a[1], sa64[2 * lr], sa64[2 * lr + 1]);
    }
    __syncthreads();
    if (env_on && P->actions != nullptr) {   // the action every robot slot of a stepping env was given
      double* rec = P->actions + (static_cast<size_t>(t) * NT + idx) * 2;
      rec[0] = sa64[2 * tid];
      rec[1] = sa64[2 * tid + 1];
    }
  }
  [[maybe_unused]] acted:

  // ---------------- phase 1: dynamics (env.py:247-277), the observation's self part
  {
    if constexpr (!ROLL) {
      r = Regs{};
      gx = 0;
      gy = 0;
      if (exists) load_state();
    }
    if (active && (DYN && A->ctl.do_dynamics) && !obsp) {
      const double d_before = sqrt((gx - r.x) * (gx - r.x) + (gy - r.y) * (gy - r.y));
      const int nc = A->s.n_cores[e];
      const double* cores = A->s.cores + static_cast<size_t>(e) * A->s.max_cores * 4;
      // the lane's action: the Actor's (LDS), or row t of the caller's
      const double* act = POL != kPolNone ? sa64 + 2 * tid : A->actions + (ROLL ? static_cast<size_t>(t) * 2 * NT : 0) + 2 * idx;
      robot_act(ParamsKArg{&A->p}, r, act[0], act[1], A->ctl.is_continuous, cores,
                nc < A->s.max_cores ? nc : A->s.max_cores);
      const double d_after = sqrt((gx - r.x) * (gx - r.x) + (gy - r.y) * (gy - r.y));
      reward = 0.0;
      reward += A->p.timestep_penalty;
      reward += d_before - d_after;
    }
    if constexpr (!ROLL) {
      if (exists && (DYN && A->ctl.do_dynamics)) store_state();
    }
    double so0 = 0, so1 = 0, so2 = 0, so3 = 0, so4 = 0;
    if (rlane) {
      sx[tid] = r.x;
      sy[tid] = r.y;
      sv0[tid] = r.v0;
      sv1[tid] = r.v1;
      soff[tid] = exists ? (deact ? 1 : 0) : 1;
      sact[tid] = active ? 1 : 0;
    }
    if (active) {
      double sn, cs;
      sincos(r.th, &sn, &cs);
      const double tx = -(cs * r.x + sn * r.y);
      const double ty = -(-sn * r.x + cs * r.y);
      scs[tid] = cs;
      ssn[tid] = sn;
      stx[tid] = tx;
      sty[tid] = ty;
      so0 = (cs * gx + sn * gy) + tx;
      so1 = (-sn * gx + cs * gy) + ty;
      so2 = cs * r.v0 + sn * r.v1;
      so3 = -sn * r.v0 + cs * r.v1;
      so4 = r.v2;
      if (sqrt((gx - r.x) * (gx - r.x) + (gy - r.y) * (gy - r.y)) <= A->p.goal_dis) reach = true;
    }
    if (env_on) {   // packed f32 obs row, self part (replay_buffer.py:51-69 + the .float() of agent.py:363-366)
      const bool a = active;
      each_out(A, [&](const AsvStepOut& o, auto opt, size_t base) {
        if (!opt || o.obs != nullptr) {
          float* of = o.obs + (idx - base) * ASVRL_OBS_DIM;
          *reinterpret_cast<float4*>(of) = a ? make_float4(static_cast<float>(so0), static_cast<float>(so1),
                                                            static_cast<float>(so2), static_cast<float>(so3))
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
          of[4] = a ? static_cast<float>(so4) : 0.f;
          of[5] = a ? static_cast<float>(r.tl) : 0.f;
          of[6] = a ? static_cast<float>(r.tr) : 0.f;
        }
        if (o.obs64 != nullptr) {
          double* ob = o.obs64 + idx * 32;
          ob[0] = a ? so0 : 0.0;
          ob[1] = a ? so1 : 0.0;
          ob[2] = a ? so2 : 0.0;
          ob[3] = a ? so3 : 0.0;
          ob[4] = a ? so4 : 0.0;
          ob[5] = a ? r.tl : 0.0;
          ob[6] = a ? r.tr : 0.0;
        }
      });
    }
  }
  if (env_on) {
    if (!ROLL || t == 0 || obsp) {   // the buoys and the counts do not change over a rollout, but for a reset
      const int no = A->s.n_obs[e];
      for (int k = i; k < O; k += R) {
        const double* ob = A->s.obstacles + (static_cast<size_t>(e) * O + k) * 3;
        double* dst = sob + (static_cast<size_t>(le) * O + k) * 3;
        if (k < no) {
          dst[0] = ob[0];
          dst[1] = ob[1];
          dst[2] = ob[2];
        }
      }
      if (i == 0) {
        sno[le] = no;
        snr[le] = nrob;
      }
    }
    if (i == 0) salive[le] = 0;
  }
  __syncthreads();
  A = kfresh(A);

  // candidate slot c of robot qi in local env qe: obstacles first, then robots (self, deactivated and
  // absent ones are not candidates, wamv.py:487-491)
  auto candidate = [&](int qe, int qi, int c, double& ox, double& oy, double& orad, double& vx0, double& vy0) {
    if (c < O) {
      if (c >= sno[qe]) return false;
      const double* ob = sob + (static_cast<size_t>(qe) * O + c) * 3;
      ox = ob[0];
      oy = ob[1];
      orad = ob[2];
      vx0 = 0.0;
      vy0 = 0.0;
      return true;
    }
    const int j = c - O;
    if (!(j < snr[qe] && j != qi && !soff[qe * R + j])) return false;
    ox = sx[qe * R + j];
    oy = sy[qe * R + j];
    orad = A->p.r;
    vx0 = sv0[qe * R + j];
    vy0 = sv1[qe * R + j];
    return true;
  };
  uint64_t ctr = A->ctl.counter + (A->ctl.counter_dev != nullptr ? *A->ctl.counter_dev : 0ull) +
                 (ROLL ? static_cast<uint64_t>(t) : 0ull);
  if constexpr (AR) {
    if (obsp) ctr = ctr - A->ctl.counter + RS->obs_counter;
  }
  // row t of the injected draws
  const size_t noise_t = (ROLL && NM == 0) ? static_cast<size_t>(t) * NT * S * 5 : 0;
  const bool full_circle = 0.5 * A->p.angle >= kPi;

  // ---------------- phase 2: one (robot, candidate) pair per lane (wamv.py:478-511)
  const KArg<PairsArgs> A_loop = A;
  for (int q = tid; q < npairs; q += BLOCK) {
    const KArg<PairsArgs> A = kfresh(A_loop);   // this iteration's parameters, not held across iterations
    const int qr = q / S;
    const int c = q - qr * S;
    const int qe = qr / R;
    const int qi = qr - qe * R;
    unsigned char flag = 0;
    double key = INFINITY;
    double ox = 0, oy = 0, orad = 0, vx0 = 0, vy0 = 0;
    if (sact[qr] && candidate(qe, qi, c, ox, oy, orad, vx0, vy0)) {
      const size_t qidx = static_cast<size_t>(bid * epb + qe) * R + qi;
      double n0, n1, n2, n3, n4;
      draw_noise<NM>(kref(A).p, kref(A).ctl, ctr, A->noise + noise_t, qidx, c, S, n0, n1, n2, n3, n4);
      pvm[q] = static_cast<VmT>(n4);
      const double cs = scs[qr], sn = ssn[qr], tx = stx[qr], ty = sty[qr];
      const double pxn = ox + n0, pyn = oy + n1;  // Perception (wamv.py:27-40)
      const double rn = A->p.r_mean_ratio * orad + (1 - A->p.r_mean_ratio) * n4 / kPi * orad;
      const double qx = (cs * pxn + sn * pyn) + tx, qy = (-sn * pxn + cs * pyn) + ty;
      const double qn = sqrt(qx * qx + qy * qy);
      bool det = qn <= A->p.range + rn;  // check_detection (wamv.py:293-303)
      if (det && !full_circle) {
        const double ang = atan2(qy, qx);
        det = !(ang < -0.5 * A->p.angle || ang > 0.5 * A->p.angle);
      }
      if (det) {
        flag = 1;
        const double rx = sx[qr], ry = sy[qr];   // check_collision (wamv.py:281-291), true positions
        const double d = sqrt((rx - ox) * (rx - ox) + (ry - oy) * (ry - oy)) - orad - A->p.r;
        if (d <= 0.0) flag |= 2;
        key = qn - rn - A->p.r;
      }
    }
    pk[q] = key;
    pfl[q] = flag;
  }
  __syncthreads();
  A = kfresh(A);

  // ---------------- phase 3: the robot's candidates in the reference's order (wamv.py:512-516)
  int cnt = -1;
  if (active) {
    double k0 = INFINITY, k1 = INFINITY, k2 = INFINITY, k3 = INFINITY, k4 = INFINITY;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    int nkept = 0;
    const int q0 = tid * S;
    for (int c = 0; c < S; ++c) {
      const unsigned char f = pfl[q0 + c];
      if (!(f & 1)) continue;
      if (f & 2) coll = true;
      double kc = pk[q0 + c];
      int cc = c;
      // heapq.nsmallest == stable ascending order: a new candidate passes equal keys
      auto ins = [&](double& kk, int& ck) {
        if (kc < kk) {
          const double tk = kk;
          const int tc = ck;
          kk = kc;
          ck = cc;
          kc = tk;
          cc = tc;
        }
      };
      ins(k0, c0);
      ins(k1, c1);
      ins(k2, c2);
      ins(k3, c3);
      ins(k4, c4);
      ++nkept;
    }
    cnt = nkept < A->p.max_obj_num ? nkept : A->p.max_obj_num;
    unsigned short* kp = skept + 5 * tid;
    kp[0] = static_cast<unsigned short>(c0);
    kp[1] = static_cast<unsigned short>(c1);
    kp[2] = static_cast<unsigned short>(c2);
    kp[3] = static_cast<unsigned short>(c3);
    kp[4] = static_cast<unsigned short>(c4);
  }
  if (rlane) scnt[tid] = static_cast<signed char>(cnt);
  // phase 4's work list: the kept objects only (about half of the 5 * nrb (robot, k) slots), placed by
  // a workgroup scan of the counts in robot order
  const int lane = tid & (kWave - 1);
  int kin = cnt > 0 ? cnt : 0;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(kin, d);
    if (lane >= d) kin += t;
  }
  if (lane == kWave - 1) swt[tid / kWave] = kin;
  __syncthreads();
  A = kfresh(A);
  int nitem = 0, ibase = 0;
#pragma unroll
  for (int w = 0; w < BLOCK / kWave; ++w) {
    ibase += w < tid / kWave ? swt[w] : 0;
    nitem += swt[w];
  }
  if (cnt > 0) {
    const int off = ibase + kin - cnt;
    for (int k = 0; k < cnt; ++k) sitem[off + k] = static_cast<unsigned short>(5 * tid + k);
  }
  __syncthreads();
  A = kfresh(A);

  // ---------------- phase 4: one lane per kept object: its observation row and COLREGs test
  const KArg<PairsArgs> A_loop4 = A;
  for (int it = tid; it < nitem; it += BLOCK) {
    const KArg<PairsArgs> A = kfresh(A_loop4);   // this iteration's parameters, not held across iterations
    const int kq = sitem[it];
    const int qr = kq / 5;
    const int k = kq - 5 * qr;
    const int qe = qr / R;
    const int qi = qr - qe * R;
    const int e2 = bid * epb + qe;
    unsigned char cf = 0;
    double ph = 0.0;
    {
      const size_t qidx = static_cast<size_t>(e2) * R + qi;
      double ra, rb, rc, rd, re;
      {
        const int c = skept[kq];
        double ox = 0, oy = 0, orad = 0, vx0 = 0, vy0 = 0;
        candidate(qe, qi, c, ox, oy, orad, vx0, vy0);
        double n0, n1, n2, n3, n4 = static_cast<double>(pvm[qr * S + c]);
        draw_noise<NM, false>(kref(A).p, kref(A).ctl, ctr, A->noise + noise_t, qidx, c, S, n0, n1, n2, n3, n4);
        const double cs = scs[qr], sn = ssn[qr], tx = stx[qr], ty = sty[qr];
        const double pxn = ox + n0, pyn = oy + n1;  // as phase 2
        const double vxn = vx0 + n2, vyn = vy0 + n3;
        const double rn = A->p.r_mean_ratio * orad + (1 - A->p.r_mean_ratio) * n4 / kPi * orad;
        ra = (cs * pxn + sn * pyn) + tx;
        rb = (-sn * pxn + cs * pyn) + ty;
        rc = cs * vxn + sn * vyn;
        rd = -sn * vxn + cs * vyn;
        re = rn;
        if (!(sqrt(rc * rc + rd * rd) < 0.5)) {   // colregs_body's first test, ahead of the call
          bool ev;
          const bool hit = colregs_ev(A->p.r, cs, sn, sv0[qr], sv1[qr], ra, rb, rc, rd, re, ph, ev);
          cf = static_cast<unsigned char>((ev ? 1 : 0) | (hit ? 2 : 0));
        }
      }
      each_out(A, [&](const AsvStepOut& o, auto opt, size_t base) {
        if (!opt || o.obs != nullptr) {
          float* of = o.obs + (qidx - base) * ASVRL_OBS_DIM + 7 + 5 * k;
          of[0] = static_cast<float>(ra);
          of[1] = static_cast<float>(rb);
          of[2] = static_cast<float>(rc);
          of[3] = static_cast<float>(rd);
          of[4] = static_cast<float>(re);
        }
        if (o.obs64 != nullptr) {
          double* ob = o.obs64 + qidx * 32 + 7 + 5 * k;
          ob[0] = ra;
          ob[1] = rb;
          ob[2] = rc;
          ob[3] = rd;
          ob[4] = re;
        }
      });
    }
    pfl[kq] = cf;
    pk[kq] = ph;
  }
  __syncthreads();
  A = kfresh(A);

  // ---------------- phase 5: COLREGs in order (wamv.py:517-521), reward / done / info, bookkeeping
  bool apply = false;
  if constexpr (!ROLL) phi = exists ? A->s.rs[ASVRL_F_PHI * NT + idx] : 0.0;
  for (int k = 0; k < cnt; ++k) {   // the serial chain: phi of every evaluated object up to the first hit
    const unsigned char f = pfl[5 * tid + k];
    if (f & 1) phi = pk[5 * tid + k];
    if (f & 2) {
      apply = true;
      break;
    }
  }
  if constexpr (!ROLL) ret = exists ? A->s.rs[ASVRL_F_RET * NT + idx] : 0.0;
  AsvStepCtl cobs{};   // AR: the observation pass's control (do_dynamics, trainer_deactivate, gamma: 0)
  if constexpr (AR) {
    if (!obsp) {
      cobs.do_dynamics = A->ctl.do_dynamics;
      cobs.trainer_deactivate = A->ctl.trainer_deactivate;
      cobs.gamma = A->ctl.gamma;
    }
  }
  const StepResult res = step_result(kref(A).p, AR ? cobs : kref(A).ctl, exists, deact, active, ep_ts, fl, coll, reach, apply, phi, reward,
                                     ret);
  if (A->ctl.trainer_deactivate && (DYN && A->ctl.do_dynamics) && !obsp && exists && !(res.nfl & ASVRL_FLAG_DEACTIVATED))
    atomicAdd(&salive[le], 1);
  if constexpr (AR) {   // the step's rows a replay push takes (obj_cnt >= 0), a wave's count in one atomic
    if (!obsp && RS->pushed != nullptr) {
      const unsigned long long bal = __ballot(exists && cnt >= 0);
      if ((tid & (kWave - 1)) == 0 && bal != 0) atomicAdd(RS->pushed + t, static_cast<int32_t>(__popcll(bal)));
    }
  }
  if (exists) {
    if constexpr (!ROLL) {
      if ((DYN && A->ctl.do_dynamics)) A->s.rs[ASVRL_F_RET * NT + idx] = res.ret;
      A->s.rs[ASVRL_F_PHI * NT + idx] = phi;
      A->s.rflags[idx] = res.nfl;
    } else {
      // kept for the next step, and where the env's lane 0 sums an ended episode (env_end_from): this lane's
      // first (robot, k) slot, whose phase 4 values the chain above has read
      ret = res.ret;
      flv = res.nfl;
      pk[5 * tid] = res.ret;
      pfl[5 * tid] = res.nfl;
    }
  }
  if (env_on) {
    const bool a = active;
    each_out(A, [&](const AsvStepOut& o, auto opt, size_t base) {
      if (!opt || o.obs != nullptr) {
        float4* o4 = reinterpret_cast<float4*>(o.obs + (idx - base) * ASVRL_OBS_DIM);
        for (int k = cnt > 0 ? cnt : 0; k < 5; ++k) {   // the object rows phase 4 did not write
          float* of = o.obs + (idx - base) * ASVRL_OBS_DIM + 7 + 5 * k;
          of[0] = 0.f;
          of[1] = 0.f;
          of[2] = 0.f;
          of[3] = 0.f;
          of[4] = 0.f;
        }
        o4[8] = make_float4((a && cnt > 0) ? 1.f : 0.f, (a && cnt > 1) ? 1.f : 0.f, (a && cnt > 2) ? 1.f : 0.f,
                            (a && cnt > 3) ? 1.f : 0.f);
        o4[9] = make_float4((a && cnt > 4) ? 1.f : 0.f, 0.f, 0.f, 0.f);
      }
      if (o.obs64 != nullptr) {
        for (int k = cnt > 0 ? cnt : 0; k < 5; ++k) {
          double* ob = o.obs64 + idx * 32 + 7 + 5 * k;
          ob[0] = 0.0;
          ob[1] = 0.0;
          ob[2] = 0.0;
          ob[3] = 0.0;
          ob[4] = 0.0;
        }
      }
      if (!opt || o.obj_cnt != nullptr) o.obj_cnt[idx] = static_cast<int8_t>(exists ? cnt : -1);
      if (!opt || o.reward != nullptr) o.reward[idx] = res.reward;
      if (!opt || o.done != nullptr) o.done[idx] = res.done;
      if (!opt || o.info != nullptr) o.info[idx] = res.info;
    });
  }
  __syncthreads();
  A = kfresh(A);
  if constexpr (AR) {
    if (obsp) {
      // the observation pass's own state writes (phi of its COLREGs chain, the flags), kept in registers until the
      // window's last step
      if (exists && t == n_steps - 1) {
        A->s.rs[ASVRL_F_PHI * NT + idx] = phi;
        A->s.rflags[idx] = flv;
      }
      continue;   // the next step
    }
  }
  if constexpr (!ROLL) {
    if (env_on && i == 0 && (DYN && A->ctl.do_dynamics)) env_end(kref(A).p, kref(A).s, kref(A).ctl, kref(A).out, e, ep_ts, nrob, salive[le], NT);
  } else {
    // the env's end (trainer.py:172), by its lane 0 for the totals and by every lane of a held or auto-resetting
    // rollout
    const KArg<AsvRollout> Q = kfresh(RO);
    bool end = false;
    if (env_on && A->ctl.trainer_deactivate && (hold || AR || i == 0))
      end = (ep_ts >= A->p.episode_limit) || salive[le] == 0;
    if (env_on && i == 0) {
      env_end_from(kref(A).p, kref(A).s, kref(A).ctl, kref(A).out, e, ep_ts, nrob, salive[le],
                   [&](int j) { return pk[5 * (le * R + j)]; }, [&](int j) { return pfl[5 * (le * R + j)]; });
      if (Q->env_done != nullptr) Q->env_done[static_cast<size_t>(t) * A->s.n_envs + e] = end ? 1 : 0;
    }
    // the state goes back to HBM after the env's last step
    // (AR: and in front of the env's reset, whose sampler leaves the rows of robot slots it does not fill as they are)
    if (exists && (t == n_steps - 1 || ((hold || AR) && end))) {
      store_state();
      A->s.rs[ASVRL_F_RET * NT + idx] = ret;
      A->s.rs[ASVRL_F_PHI * NT + idx] = phi;
      A->s.rflags[idx] = flv;
    }
    if (exists && Q->rs != nullptr) {
      double* q = Q->rs + static_cast<size_t>(t) * ASVRL_NUM_FIELDS * NT + idx;
      const double v[ASVRL_NUM_FIELDS] = {r.x, r.y, r.th, r.vr0, r.vr1, r.vr2, r.v0, r.v1, r.v2, r.tl, r.tr,
                                          r.lp, r.rp, gx, gy, phi, ret};
#pragma unroll
      for (int f = 0; f < ASVRL_NUM_FIELDS; ++f) q[f * NT] = v[f];
    }
    if (env_on) {
      ++ep_ts;
      ++taken;
    }
    if (hold && end) on = false;
    if constexpr (AR) {
      // ---------------- the ended envs restart (see the comment in front of this function for the barriers)
      rstl = env_on && end;
      int* srst = reinterpret_cast<int*>(ar_lds + (BLOCK / kWave) * sizeof(ResetLds));   // [epb] env le was reset
      if (rlane && i == 0) srst[le] = rstl ? 1 : 0;
      if (!__syncthreads_or(rstl ? 1 : 0)) continue;   // workgroup-uniform: no env of the group ended in this step
      // the ended envs' state stores above (and the flags in LDS) before the resetting waves' reads and stores
      __syncthreads();
      {
        const KArg<AsvAutoReset> Z = kfresh(RS);
        const uint64_t rctr = Z->reset_counter + (A->ctl.counter_dev != nullptr ? *A->ctl.counter_dev : 0ull) +
                              static_cast<uint64_t>(t);
        const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
        ResetLds* W = reinterpret_cast<ResetLds*>(ar_lds);
        // one wave per env, the waves taking the group's envs in turn (qe and the flag are wave-uniform)
        for (int qe = wv; qe < epb; qe += BLOCK / kWave)
          if (__builtin_amdgcn_readfirstlane(srst[qe]) != 0)
            reset_env(kref(A).p, kref(A).s, kref(Z).cfg, bid * epb + qe, A->ctl.seed, rctr, tid & (kWave - 1), W[wv]);
      }
      __syncthreads();   // the resets' global writes (workgroup-scope release / acquire) before the reloads below
      A = kfresh(A);
      if (rstl) {   // what the rollout keeps over the steps, from the reset state
        nrob = A->s.n_robots[e];
        exists0 = i < nrob;
        r = Regs{};
        gx = 0;
        gy = 0;
        phi = 0.0;
        ret = 0.0;
        flv = 0;
        if (exists0) {
          load_state();
          phi = A->s.rs[ASVRL_F_PHI * NT + idx];
          ret = A->s.rs[ASVRL_F_RET * NT + idx];
          flv = A->s.rflags[idx];
        }
        ep_ts = 0;
        if (i == 0) ++nreset;
      }
      // the observation pass of the reset envs (it restages their buoys and counts)
      obsp = true;
      goto phases;
    }
  }
  }   // step t
  if constexpr (ROLL) {
    if (lane_env && i == 0 && RO->steps_run != nullptr) RO->steps_run[e] = taken;
  }
  if constexpr (AR) {
    if (lane_env && i == 0 && RS->resets != nullptr) RS->resets[e] = nreset;
  }
}


// The step kernel: workgroup b takes env group group0 + b (a step may be split into launches of at most
// AsvEnvLaunch.max_groups workgroups, one after another: the rollout's share of the chip beside the learner).
// XCD-aware: the dispatcher deals workgroups to the eight XCDs round-robin, so consecutive env groups --
// whose state / observation rows share cache lines at their edges -- would sit in different L2s and each
// write back its part of the shared lines; the bijection below gives each XCD a contiguous run of groups.
// Measured alternative, removed (workgroup x = group x): time neutral (2^18 envs 441.3 / 442.8 -> 444.2 /
// 443.4 us, 4096 envs 26.7 us either way), counter reads 302 -> 282 MB per plateau launch with the bijection
// (profiles/r05bd_env_xcd_swizzle_ab.txt).
__device__ __forceinline__ int xcd_group(int x, int n) {
  constexpr int kXcd = 8;
  const int q = n / kXcd, rr = n % kXcd, xcd = x % kXcd, k = x / kXcd;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + k;
}
template <int BLOCK, int NM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(NM == 1 ? 1 : ASVRL_ENV_PAIRS_WPE))) void env_pairs_kernel(PairsArgs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const KArg<PairsArgs> A = kargs<PairsArgs>();
  env_pairs_block<BLOCK, NM>(A, A->epb,
                             A->group0 + xcd_group(static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x)), smem);
}

// The rollout windows: K steps in one launch, one kernel instantiation per policy x auto-reset (x block x noise
// mode). Their one argument: the step's, the window's, then the policy's struct (closed loop), then the auto-reset's
// and where its LDS starts in the dynamic carve (AR). A member a kernel does not take is an empty struct that
// occupies nothing, so each instantiation's kernarg segment holds exactly the members it reads, in this order.
struct NoPolicy {};   // the open loop: the actions out of ro
template <int> struct Absent {};
template <class Pol, bool AR>
struct WindowArgs {
  PairsArgs k;   // noise: row 0 of the rollout's; actions: row 0 of the rollout's (open loop), null (closed loop)
  AsvRollout ro;
  [[no_unique_address]] std::conditional_t<std::is_same_v<Pol, NoPolicy>, Absent<0>, Pol> pi;
  [[no_unique_address]] std::conditional_t<AR, AsvAutoReset, Absent<1>> ar;
  [[no_unique_address]] std::conditional_t<AR, int, Absent<2>> ar_off;
};
static_assert(sizeof(WindowArgs<NoPolicy, false>) == sizeof(PairsArgs) + sizeof(AsvRollout) &&
                  sizeof(WindowArgs<AsvPolicy, false>) == sizeof(WindowArgs<NoPolicy, false>) + sizeof(AsvPolicy) &&
                  sizeof(WindowArgs<NoPolicy, true>) == sizeof(WindowArgs<NoPolicy, false>) + sizeof(AsvAutoReset) + 8,
              "absent members take no room in the kernarg segment");

// K open-loop steps (asvrl_env_rollout, asvrl_env_rollout_ar): env_pairs_kernel's workgroup-to-group mapping and LDS
// carve, the step loop inside the workgroup (env_pairs_block<ROLL>). An env group needs nothing from another
// group, so no step waits on the rest of the grid. Two waves per SIMD by registers: the resident state rides
// through the pair phases, and the training shape (4096 envs x 5 robots: 512 workgroups of 4 waves on 1024
// SIMDs) has no more than two waves per SIMD to place.
// AR: the auto-reset in the step loop (env_pairs_block<AR>), with the waves' ResetLds and the per-env reset flags at
// ar_off of the dynamic LDS, behind everything the plain kernel carves. Philox noise only: no NM = 0 instantiation.
#ifndef ASVRL_ENV_ROLLOUT_WPE
#define ASVRL_ENV_ROLLOUT_WPE 2
#endif
template <int BLOCK, int NM, bool AR>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(NM == 1 ? 1 : ASVRL_ENV_ROLLOUT_WPE))) void env_rollout_kernel(WindowArgs<NoPolicy, AR>) {
  static_assert(!AR || NM != 0, "the auto-reset is Philox noise only");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const KArg<WindowArgs<NoPolicy, AR>> RA = kargs<WindowArgs<NoPolicy, AR>>();
  const int epb = RA->k.epb, bid = RA->k.group0 + xcd_group(static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x));
  if constexpr (AR)
    env_pairs_block<BLOCK, NM, true, true, kPolNone, true>(&RA->k, epb, bid, smem, &RA->ro, nullptr, nullptr,
                                                           &RA->ar, smem + RA->ar_off);
  else
    env_pairs_block<BLOCK, NM, true, true>(&RA->k, epb, bid, smem, &RA->ro);
}

// K closed-loop steps (asvrl_policy_rollout, asvrl_dqn_rollout, asvrl_sac_rollout and their _ar forms):
// env_rollout_kernel with the policy POL in front of every step (env_pairs_block<POL>). The trunk's weight images
// (bf16: 112 KB, 115 KB with the f32 biases and the output layer) sit in the static ActorLds beside the pair carve,
// the workgroup's observation rows (160 B per robot) and action pairs (16 B per robot), so one workgroup owns a CU:
// one wave per SIMD and the whole register file. kPolDqn: the head's 8 KB image and its bias stay in L2. kPolSac:
// the f32 head beside the trunk (SacHeadLds, 2064 B: 512 weights every lane reads per tile, so they sit in LDS, not
// L2); no other policy's kernel declares it.
#ifndef ASVRL_ENV_POLICY_WPE
#define ASVRL_ENV_POLICY_WPE 1, 1
#endif
template <int BLOCK, int NM, int POL, bool AR>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(ASVRL_ENV_POLICY_WPE))) void env_policy_rollout_kernel(WindowArgs<typename PolicyOf<POL>::type, AR>) {
  static_assert(POL != kPolNone, "the open loop is env_rollout_kernel");
  static_assert(!AR || NM != 0, "the auto-reset is Philox noise only");
  using Args = WindowArgs<typename PolicyOf<POL>::type, AR>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ __attribute__((aligned(16))) atile::ActorLds AL;
  sactile::SacHeadLds* head = nullptr;
  if constexpr (POL == kPolSac) {
    __shared__ __attribute__((aligned(16))) sactile::SacHeadLds HL;
    head = &HL;
  }
  const KArg<Args> PA = kargs<Args>();
  const int epb = PA->k.epb, bid = PA->k.group0 + xcd_group(static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x));
  if constexpr (AR)
    env_pairs_block<BLOCK, NM, true, true, POL, true>(&PA->k, epb, bid, smem, &PA->ro, &PA->pi, &AL, &PA->ar,
                                                      smem + PA->ar_off, head);
  else
    env_pairs_block<BLOCK, NM, true, true, POL>(&PA->k, epb, bid, smem, &PA->ro, &PA->pi, &AL, nullptr, nullptr,
                                                head);
}

// The K-launch fallback of the _ar calls. In front of step t: row t of obs_prev, the observation (src) the stepping
// envs' rows hold ...
__global__ __launch_bounds__(kBlock) void autoreset_obs_prev_kernel(const float* __restrict__ src, float* __restrict__ row,
                                                                    const uint8_t* __restrict__ mask, int n_envs, int R) {
  constexpr int kQ = ASVRL_OBS_DIM / 4;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_envs * R * kQ) return;
  if (mask != nullptr && mask[q / (R * kQ)] == 0) return;
  reinterpret_cast<float4*>(row)[q] = reinterpret_cast<const float4*>(src)[q];
}
// ... and behind it, one lane per env: the reset mask (the env stepped and its episode ended), formed on the
// device, and the window's counts
__global__ __launch_bounds__(kBlock) void autoreset_mask_kernel(const uint8_t* __restrict__ env_done,
                                                                const uint8_t* __restrict__ mask,
                                                                const int8_t* __restrict__ obj_cnt, int n_envs, int R,
                                                                uint8_t* __restrict__ reset_mask, int32_t* resets,
                                                                int32_t* pushed_t) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_envs) return;
  const bool on = mask == nullptr || mask[e] != 0;
  const bool rst = on && env_done[e] != 0;
  reset_mask[e] = rst ? 1 : 0;
  if (rst && resets != nullptr) resets[e] += 1;
  if (on && pushed_t != nullptr) {
    int c = 0;
    for (int i = 0; i < R; ++i) c += obj_cnt[static_cast<size_t>(e) * R + i] >= 0 ? 1 : 0;
    if (c != 0) atomicAdd(pushed_t, c);
  }
}

// The sweep fallback of asvrl_policy_rollout: the step count of its t-th act launch, *src + t, into the call's
// scratch (the caller's counter is never written) ...
__global__ void policy_step_count_kernel(const int64_t* src, int64_t* dst, int t) {
  *dst = (src != nullptr ? *src : 0) + t;
}
// ... and the actions of the envs that take step t into row t of the record
__global__ __launch_bounds__(kBlock) void policy_actions_kernel(const double* __restrict__ act, double* __restrict__ row,
                                                                const uint8_t* __restrict__ mask, int n_envs, int R) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_envs * R) return;
  if (mask != nullptr && mask[k / R] == 0) return;
  row[2 * k] = act[2 * k];
  row[2 * k + 1] = act[2 * k + 1];
}

// The sweep layout's rollout is K single launches (asvrl_env_rollout); after step t this kernel, one lane per
// env, copies the step's outputs and state into row t of the kept records, counts the env's steps and, for
// hold_done, clears the mask of an env whose episode ended.
__global__ __launch_bounds__(kBlock) void rollout_record_kernel(AsvEnvState s, AsvStepOut out, AsvRollout ro, int t,
                                                                const uint8_t* mask, uint8_t* hold_mask) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n_envs) return;
  if (mask != nullptr && mask[e] == 0) return;
  const int R = s.max_robots;
  const size_t NT = static_cast<size_t>(s.n_envs) * R;
  const size_t t0 = static_cast<size_t>(t) * NT;
  const int nrob = s.n_robots[e];
  for (int i = 0; i < R; ++i) {
    const size_t idx = static_cast<size_t>(e) * R + i;
    if (ro.reward != nullptr) ro.reward[t0 + idx] = out.reward[idx];
    if (ro.done != nullptr) ro.done[t0 + idx] = out.done[idx];
    if (ro.info != nullptr) ro.info[t0 + idx] = out.info[idx];
    if (ro.obj_cnt != nullptr) ro.obj_cnt[t0 + idx] = out.obj_cnt[idx];
    if (ro.obs != nullptr)
      for (int k = 0; k < ASVRL_OBS_DIM; ++k) ro.obs[(t0 + idx) * ASVRL_OBS_DIM + k] = out.obs[idx * ASVRL_OBS_DIM + k];
    if (ro.rs != nullptr && i < nrob)
      for (int f = 0; f < ASVRL_NUM_FIELDS; ++f) ro.rs[(static_cast<size_t>(t) * ASVRL_NUM_FIELDS + f) * NT + idx] = s.rs[f * NT + idx];
  }
  if (ro.env_done != nullptr) ro.env_done[static_cast<size_t>(t) * s.n_envs + e] = out.env_done[e];
  if (ro.steps_run != nullptr) ro.steps_run[e] += 1;
  if (hold_mask != nullptr && out.env_done[e] != 0) hold_mask[e] = 0;
}

// ------------------------------------------------------------------ reset (env.py:72-164)
__device__ inline bool far_enough(double ax, double ay, double bx, double by, double lim, bool strict) {
  const double dx = ax - bx, dy = ay - by;
  const double d = sqrt(dx * dx + dy * dy);
  return strict ? !(d <= lim) : !(d < lim);
}

// One wave per env being reset. Every phase is rejection sampling with at most 500 draws in
// the reference's order (robots env.py:106-120, cores :123-136 with check_core :378-418,
// obstacles :151-162 with check_obstacle :420-456). The wave draws 64 consecutive candidates at
// once (candidate c's values come from its own Philox counter (c, env, phase, step), not from a
// shared stream) and tests each against everything accepted so far; then, while the batch holds a
// valid one, it accepts the lowest-numbered (ballot), broadcasts its values (v_readlane) and drops the
// candidates before it and those conflicting with it -- the same accepted sequence as testing the
// candidates one by one (a rejected candidate stays rejected as the accepted set grows; a later one is
// valid iff it is valid against the old set and the new member). Each batch's draws and tests against
// the set are made once (round 4's kernel restarted the batch after every acceptance, redrawing and
// retesting up to 63 candidates each time). The accepted set of the phase lives in LDS for the phases
// after it. Restated one candidate at a time by oracle/asv_oracle.c or_device_reset (bit-identical:
// tests/test_env_kernel_gpu.py).
struct CandDraw {
  uint32_t k0, k1, e, ctr;
  __device__ double u(int phase, int cand, int j) const {   // j-th double of candidate cand
    const U4 r = philox4x32_10(U4{static_cast<uint32_t>(cand) * 4u + static_cast<uint32_t>(j >> 1), e,
                                  static_cast<uint32_t>(phase), ctr}, k0, k1);
    const uint64_t hi = (j & 1) ? r.z : r.x, lo = (j & 1) ? r.w : r.y;
    const uint64_t bits = ((hi << 32) | lo) >> 11;
    return (static_cast<double>(bits) + 1.0) * (1.0 / 9007199254740992.0);
  }
  // both doubles of one Philox call (j = 2 p, 2 p + 1)
  __device__ void u2(int phase, int cand, int p, double& a, double& b) const {
    const U4 r = philox4x32_10(U4{static_cast<uint32_t>(cand) * 4u + static_cast<uint32_t>(p), e,
                                  static_cast<uint32_t>(phase), ctr}, k0, k1);
    a = (static_cast<double>(((static_cast<uint64_t>(r.x) << 32) | r.y) >> 11) + 1.0) * (1.0 / 9007199254740992.0);
    b = (static_cast<double>(((static_cast<uint64_t>(r.z) << 32) | r.w) >> 11) + 1.0) * (1.0 / 9007199254740992.0);
  }
};

// lane f's value (f wave-uniform, from a ballot) in every lane
__device__ __forceinline__ double bcast(double v, int f) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(u), f);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(u >> 32), f);
  return __builtin_bit_cast(double, (static_cast<uint64_t>(hi) << 32) | lo);
}

// check_core (env.py:378-418) of candidate (cx, cy, cw, Gamma) against accepted core (qx, qy, qw, qG):
// true when they conflict
__device__ __forceinline__ bool core_conflict(const AsvResetCfg& cfg, double core_r, double qx, double qy, double qw,
                                              double qG, double cx, double cy, double cw, double Gamma) {
  const double dx = qx - cx, dy = qy - cy;
  const double dis = sqrt(dx * dx + dy * dy);
  if (qw == cw) {
    const double bi = qG / (2 * kPi * cfg.v_rel_max);
    const double bj = Gamma / (2 * kPi * cfg.v_rel_max);
    return dis < bi + bj;
  }
  const double gl = fmax(qG, Gamma), gs = fmin(qG, Gamma);
  const double v1 = gl / (2 * kPi * (dis - 2 * core_r));
  const double v2 = gs / (2 * kPi * core_r);
  return v1 > cfg.p_rel * v2;
}

// env e's reset by one wave (lane = its lane index)
__device__ __forceinline__ void reset_env(const AsvParams& p, const AsvEnvState& s, const AsvResetCfg& cfg, int e,
                                          uint64_t seed, uint64_t ctr, int lane, ResetLds& W) {
  double (*srob)[kResetMaxR] = W.rob;
  double (*score)[4] = W.core;
  double (*sobs)[3] = W.obs;
  const int R = s.max_robots, O = s.max_obs, Cmax = s.max_cores;
  const size_t NT = static_cast<size_t>(s.n_envs) * R;
  double* rs = s.rs;
  const uint64_t key = seed ^ (ctr >> 32) * 0x9E3779B97F4A7C15ull;
  const CandDraw g{static_cast<uint32_t>(key), static_cast<uint32_t>(key >> 32), static_cast<uint32_t>(e),
                   static_cast<uint32_t>(ctr)};
  constexpr int kDraws = 500;

  // ---- robots
  const int want_r = cfg.num_robots < R ? cfg.num_robots : R;
  int nr = 0;
  for (int base = 0; nr < want_r && base < kDraws; base += kWave) {
    const int c = base + lane;
    double u0, u1, u2, u3;
    g.u2(0, c, 0, u0, u1);
    g.u2(0, c, 1, u2, u3);
    const double sxv = 2.0 + (cfg.width - 4.0) * (1.0 - u0);
    const double syv = 2.0 + (cfg.height - 4.0) * (1.0 - u1);
    const double gxv = 2.0 + (cfg.width - 4.0) * (1.0 - u2);
    const double gyv = 2.0 + (cfg.height - 4.0) * (1.0 - u3);
    bool ok = c < kDraws && far_enough(gxv, gyv, sxv, syv, cfg.min_start_goal_dis, false);  // env.py:361
    for (int k = 0; k < nr && ok; ++k)
      ok = far_enough(srob[0][k], srob[1][k], sxv, syv, cfg.clear_r, true) &&
           far_enough(srob[2][k], srob[3][k], gxv, gyv, cfg.clear_r, true);
    while (nr < want_r) {
      const uint64_t bal = __ballot(ok);
      if (bal == 0) break;
      const int f = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<unsigned long long>(bal)) - 1);
      const double fx = bcast(sxv, f), fy = bcast(syv, f), fgx = bcast(gxv, f), fgy = bcast(gyv, f);
      if (lane == f) {
        srob[0][nr] = sxv;
        srob[1][nr] = syv;
        srob[2][nr] = gxv;
        srob[3][nr] = gyv;
        const size_t id = static_cast<size_t>(e) * R + nr;
        rs[ASVRL_F_X * NT + id] = sxv;  // reset_robot / reset_state (env.py:166-176, wamv.py:177-193)
        rs[ASVRL_F_Y * NT + id] = syv;
        rs[ASVRL_F_GX * NT + id] = gxv;
        rs[ASVRL_F_GY * NT + id] = gyv;
        rs[ASVRL_F_THETA * NT + id] = kTwoPi * (1.0 - g.u(0, c, 4));
        for (int fld = ASVRL_F_VR0; fld <= ASVRL_F_RP; ++fld) rs[fld * NT + id] = 0.0;
        rs[ASVRL_F_PHI * NT + id] = 0.0;
        rs[ASVRL_F_RET * NT + id] = 0.0;
        s.rflags[id] = 0;
      }
      ok = ok && lane > f && far_enough(fx, fy, sxv, syv, cfg.clear_r, true) &&
           far_enough(fgx, fgy, gxv, gyv, cfg.clear_r, true);
      ++nr;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the batch's LDS rows before the next batch's reads
    __builtin_amdgcn_wave_barrier();
  }
  for (int k = nr + lane; k < R; k += kWave) s.rflags[static_cast<size_t>(e) * R + k] = ASVRL_FLAG_DEACTIVATED;

  // ---- vortex cores (env.py:123-136, check_core :378-418)
  double* cores = s.cores + static_cast<size_t>(e) * Cmax * 4;
  const int want_c = cfg.num_cores < Cmax ? cfg.num_cores : Cmax;
  int nc = 0;
  for (int base = 0; nc < want_c && base < kDraws; base += kWave) {
    const int c = base + lane;
    double u0, u1, u2, u3;
    g.u2(1, c, 0, u0, u1);
    g.u2(1, c, 1, u2, u3);
    const double cx = cfg.width * (1.0 - u0);
    const double cy = cfg.height * (1.0 - u1);
    const double cw = u2 <= 0.5 ? 1.0 : 0.0;
    const double ve = cfg.v_lo + (cfg.v_hi - cfg.v_lo) * (1.0 - u3);
    const double Gamma = 2 * kPi * p.core_r * ve;
    bool ok = c < kDraws && !(cx - p.core_r < 0.0 || cx + p.core_r > cfg.width) &&
              !(cy - p.core_r < 0.0 || cy + p.core_r > cfg.width);  // (sic) env.py:383
    for (int k = 0; k < nr && ok; ++k)
      ok = far_enough(cx, cy, srob[0][k], srob[1][k], p.core_r + cfg.clear_r, false) &&
           far_enough(cx, cy, srob[2][k], srob[3][k], p.core_r + cfg.clear_r, false);
    for (int k = 0; k < nc && ok; ++k)
      ok = !core_conflict(cfg, p.core_r, score[k][0], score[k][1], score[k][2], score[k][3], cx, cy,
                          cw, Gamma);
    while (nc < want_c) {
      const uint64_t bal = __ballot(ok);
      if (bal == 0) break;
      const int f = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<unsigned long long>(bal)) - 1);
      const double fx = bcast(cx, f), fy = bcast(cy, f), fw = bcast(cw, f), fG = bcast(Gamma, f);
      if (lane == f) {
        score[nc][0] = cores[4 * nc] = cx;
        score[nc][1] = cores[4 * nc + 1] = cy;
        score[nc][2] = cores[4 * nc + 2] = cw;
        score[nc][3] = cores[4 * nc + 3] = Gamma;
      }
      ok = ok && lane > f && !core_conflict(cfg, p.core_r, fx, fy, fw, fG, cx, cy, cw, Gamma);
      ++nc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }

  // ---- static obstacles (env.py:151-162, check_obstacle :420-456)
  double* obs = s.obstacles + static_cast<size_t>(e) * O * 3;
  const int want_o = cfg.num_obs < O ? cfg.num_obs : O;
  int no = 0;
  for (int base = 0; no < want_o && base < kDraws; base += kWave) {
    const int c = base + lane;
    double u0, u1, u2, u3;
    g.u2(2, c, 0, u0, u1);
    g.u2(2, c, 1, u2, u3);
    const double ox = 5.0 + (cfg.width - 10.0) * (1.0 - u0);
    const double oy = 5.0 + (cfg.height - 10.0) * (1.0 - u1);
    const double orad = cfg.obs_r_lo + (cfg.obs_r_hi - cfg.obs_r_lo) * (1.0 - u2);
    bool ok = c < kDraws && !(ox - orad < 0.0 || ox + orad > cfg.width) && !(oy - orad < 0.0 || oy + orad > cfg.height);
    for (int k = 0; k < nr && ok; ++k)
      ok = far_enough(ox, oy, srob[0][k], srob[1][k], orad + cfg.clear_r, false) &&
           far_enough(ox, oy, srob[2][k], srob[3][k], orad + cfg.clear_r, false);
    for (int k = 0; k < nc && ok; ++k) ok = far_enough(score[k][0], score[k][1], ox, oy, p.core_r + orad, true);
    for (int k = 0; k < no && ok; ++k) ok = far_enough(sobs[k][0], sobs[k][1], ox, oy, sobs[k][2] + orad, true);
    while (no < want_o) {
      const uint64_t bal = __ballot(ok);
      if (bal == 0) break;
      const int f = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<unsigned long long>(bal)) - 1);
      const double fx = bcast(ox, f), fy = bcast(oy, f), fr = bcast(orad, f);
      if (lane == f) {
        sobs[no][0] = obs[3 * no] = ox;
        sobs[no][1] = obs[3 * no + 1] = oy;
        sobs[no][2] = obs[3 * no + 2] = orad;
      }
      ok = ok && lane > f && far_enough(fx, fy, ox, oy, fr + orad, true);
      ++no;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    s.n_robots[e] = nr;
    s.n_cores[e] = nc;
    s.n_obs[e] = no;
    s.ep_ts[e] = 0;
  }
}

__global__ __launch_bounds__(kResetWaves * kWave) void env_reset_kernel(AsvParams p, AsvEnvState s, AsvResetCfg cfg,
                                                                        const uint8_t* __restrict__ mask,
                                                                        uint64_t seed, uint64_t counter,
                                                                        const uint64_t* __restrict__ counter_dev) {
  __shared__ ResetLds W[kResetWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int e = blockIdx.x * kResetWaves + wv;
  if (e >= s.n_envs) return;                     // wave-uniform exits
  if (mask != nullptr && mask[e] == 0) return;
  reset_env(p, s, cfg, e, seed, counter + (counter_dev != nullptr ? *counter_dev : 0ull), lane, W[wv]);
}

// The training loop's auto-reset in ONE launch (asvrl_env_reset_observe): workgroup e is one wave; if env e
// ended its episode (mask), the wave resets it (reset_env) and then computes its reset observation with the
// step kernel's own phases (env_pairs_block, one env per workgroup, do_dynamics = 0): the same values as
// asvrl_env_reset followed by the masked asvrl_env_step pass, without the second launch over every env.
struct ResetObsArgs {
  PairsArgs k;   // actions / noise null, epb 1
  AsvResetCfg cfg;
  const uint8_t* mask;
  uint64_t seed, counter;
  const uint64_t* counter_dev;
};
template <int NM>
__global__ __launch_bounds__(kWave) void env_reset_observe_kernel(ResetObsArgs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // env_pairs_block's carve
  __shared__ ResetLds W;
  const KArg<ResetObsArgs> RA = kargs<ResetObsArgs>();
  const ResetObsArgs& a = kref(RA);
  const int e = blockIdx.x;
  if (a.mask[e] == 0) return;                      // workgroup-uniform
  reset_env(a.k.p, a.k.s, a.cfg, e, a.seed, a.counter + (a.counter_dev != nullptr ? *a.counter_dev : 0ull),
            threadIdx.x, W);
  __syncthreads();   // the reset's global writes (workgroup-scope release / acquire) before the observation reads
  env_pairs_block<kWave, NM, false>(kfresh<PairsArgs>(&RA->k), 1, e, smem);
}

__global__ __launch_bounds__(kBlock) void current_kernel(const double* __restrict__ cores, int nc, double core_r,
                                                        const double* __restrict__ xy, int n, double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double cx, cy;
  current_at(cores, nc, core_r, xy[2 * k], xy[2 * k + 1], cx, cy);
  out[3 * k] = cx;
  out[3 * k + 1] = cy;
  out[3 * k + 2] = 0.0;
}

}  // namespace

size_t env_sweep_smem(int R, int O) {
  const int blk = step_block(R);
  const int epb = blk / R;
  return sizeof(double) * (4 * blk + static_cast<size_t>(epb) * O * 3) + sizeof(int) * epb + blk;
}

// the pair-parallel launch: workgroup size from the pair count, envs per workgroup so that the
// pairs fill it (at least one env); AsvEnvLaunch may set the block and the envs per workgroup
struct PairLaunch {
  int blk, epb;
  size_t smem;
};
PairLaunch pair_launch(int R, int O, int n_envs, int blk_req, int epb_req, int vm_bytes) {
  const int np1 = R * (O + R);
  PairLaunch L;
  // Launch-shape rule (tools/env_try.sh, profiles/r02_env_pairs_v2_sweep*.jsonl; the kernel holds 4
  // waves per SIMD by registers, so the shape sets LDS use, tail waste and per-workgroup overheads):
  //  - up to 8 robots per env, below 16384 envs: 256-lane workgroups of about 40 robots (R = 5: 8 envs,
  //    27 us at 4096 envs vs 31-42 us for the other shapes)
  //  - up to 8 robots, from 16384 envs: one-wave workgroups of about 40 robots (R = 5: 8 envs; 416-422 us
  //    at 2^18 envs vs 428-440 us for 128/256 lanes)
  //  - more robots: 256-lane workgroups of about 120 robots (R = 17: 7 envs, 61 us at 4096 envs vs 70 us
  //    for 3 envs and 74-124 us for the other shapes)
  const bool large = n_envs >= 16384 && R <= 8;
  L.blk = (blk_req == 64 || blk_req == 128 || blk_req == 256) ? blk_req : (large ? 64 : 256);
  if (R > L.blk) L.blk = 256;
  if (R <= 8)
    L.epb = large ? 40 / R : ((40 + R - 1) / R < 64 / R ? (40 + R - 1) / R : 64 / R);
  else
    L.epb = 120 / R > 1 ? 120 / R : 1;
  if (epb_req > 0) L.epb = epb_req;
  if (L.epb * R > L.blk) L.epb = L.blk / R;
  // env_pairs_kernel's carve: 8 per-robot f64 arrays, the per-pair keys (reused as phase 4's phi),
  // obstacles, the per-pair radius draws (f32 for noise mode 2), 3 ints per env and one per wave, 5 kept
  // slots and 5 work-list entries (u16) per robot, then bytes (pair / COLREGs flags, 2 per-robot flags,
  // kept count)
  const size_t nrb = static_cast<size_t>(L.epb) * R;
  const size_t np = static_cast<size_t>(L.epb) * np1;
  const size_t nslot = np > 5 * nrb ? np : 5 * nrb;
  L.smem = sizeof(double) * (8 * nrb + nslot + static_cast<size_t>(L.epb) * O * 3) + vm_bytes * np +
           sizeof(int) * (3 * L.epb + L.blk / 64) + sizeof(unsigned short) * 10 * nrb + nslot + 3 * nrb;
  return L;
}

}  // namespace asvrl

using namespace asvrl;

// ------------------------------------------------------------------ the env step and its rollout calls
// One host path. Each call is: env_checks (its arguments), env_plan (the launch shape, and whether the
// pair-parallel kernel is taken), then launch_groups (that kernel) or, for the rollouts, rollout_fallback (K single
// steps). A rollout call is one instantiation of rollout_call per policy x auto-reset: the policy is the type of its
// one policy pointer (NoPolicy: the open loop), and what differs between policies is PolicyTraits below.

static int env_fail(const char* who, const char* what) {
  set_error(std::string(who) + ": " + what);
  return 1;
}
#define ENV_REQUIRE(cond, what)                  \
  do {                                           \
    if (!(cond)) return env_fail(who, what);     \
  } while (0)

// One step of the K-launch fallback's act launch: n observation rows x, the f64 action pairs into act, the launch's
// step count read from *step + step_add. rec_row / env_mask: row t of the kept actions and the step's env mask, for
// the policies whose act launch writes the record itself. eps_out / eps_zero: SAC's scratch (PolicyTraits::eps_rows).
struct ActStep {
  const float* x;
  size_t n;
  double* act;
  const int64_t* step;
  int step_add, robots_per_env;
  double* rec_row;
  const uint8_t* env_mask;
  float* eps_out;
  const float* eps_zero;
};
// the rows, the step count and the policy's epsilon schedule and seed into any act launch's IO struct
template <class IO, class Pol>
static void act_schedule(IO& io, const Pol* pi, const int64_t* step) {
  io.step_dev = step;
  io.eps_steps_per_count = pi->eps_steps_per_count;
  io.eps_total = pi->eps_total;
  io.eps_fraction = pi->eps_fraction;
  io.eps_initial = pi->eps_initial;
  io.eps_final = pi->eps_final;
  io.seed = pi->seed;
}
static int mlp_images(const char* who, const AsvMlpWeights& w, const char* what) {
  ENV_REQUIRE(w.enc_frag && w.b_enc && w.w1_frag && w.w2_frag && w.b1 && w.b2 && w.wout && w.bout, what);
  return 0;
}

// What differs per policy, all of it:
//   kWindow      a fused window kernel exists (env_plan may take it); false: the fallback is the call's only form
//   kPol         that kernel's env_pairs_block<POL>
//   kHeadBytes   static LDS beside the Actor's images in it
//   kActRecords  the fallback's act launch adds step_add itself and writes the record row under the step's mask;
//                false: policy_step_count_kernel in front of it and policy_actions_kernel behind it
//   eps_rows     the fallback's extra scratch, in [n][2] f32 arrays
//   checks       is_continuous and the images, in the order the call reports them
//   act          the fallback's act launch
struct PolicyDefaults {
  static constexpr bool kWindow = true, kActRecords = false;
  static constexpr int kPol = kPolNone;
  static constexpr size_t kHeadBytes = 0;
  template <class Pol> static int eps_rows(const Pol*) { return 0; }
};
template <class Pol> struct PolicyTraits;
template <> struct PolicyTraits<NoPolicy> : PolicyDefaults {};
constexpr const NoPolicy* kOpenLoop = nullptr;   // the policy argument of the step and the open-loop calls

template <> struct PolicyTraits<AsvPolicy> : PolicyDefaults {   // the AC-IQN Actor
  static constexpr int kPol = kPolActor;
  static int checks(const char* who, const AsvStepCtl* ctl, const AsvPolicy* pi) {
    ENV_REQUIRE(ctl->is_continuous, "is_continuous must be 1 (the Actor is the continuous agent)");
    return mlp_images(who, pi->w, "null actor image");
  }
  static int act(const AsvPolicy* pi, const ActStep& s, void* stream) {
    AsvMlpIO io{};
    io.x = s.x;
    io.ldx = ASVRL_OBS_DIM;
    io.n = static_cast<int32_t>(s.n);
    io.a_out64 = s.act;
    act_schedule(io, pi, s.step);
    return asvrl_actor_forward(&pi->w, &io, atile::MLP_ACT, stream);
  }
};

template <> struct PolicyTraits<AsvDqnPolicy> : PolicyDefaults {   // DQN_Policy: the (index, 0.0) pairs into act
  static constexpr int kPol = kPolDqn;
  static int checks(const char* who, const AsvStepCtl* ctl, const AsvDqnPolicy* pi) {
    ENV_REQUIRE(!ctl->is_continuous, "is_continuous must be 0 (DQN's actions are indices)");
    if (int rc = mlp_images(who, pi->w.trunk, "null DQN image")) return rc;
    ENV_REQUIRE(pi->w.head_frag != nullptr, "null pi->w.head_frag");
    // >= 2: the tile's staging reads the first two output rows (the Actor's whole output layer)
    ENV_REQUIRE(pi->w.n_actions >= 2 && pi->w.n_actions <= ASVRL_DQN_MAX_ACTIONS, "pi->w.n_actions must be in 2..32");
    return 0;
  }
  static int act(const AsvDqnPolicy* pi, const ActStep& s, void* stream) {
    AsvDqnActIO io{};
    io.x = s.x;
    io.ldx = ASVRL_OBS_DIM;
    io.n = static_cast<int32_t>(s.n);
    io.act_out = s.act;
    io.ld_act = 2;
    act_schedule(io, pi, s.step);
    return asvrl_dqn_act(&pi->w, &io, stream);
  }
};

// SAC's sampled actor: eps_in null draws the noise in the kernel, an all-zero eps_in (deterministic) is the mean
// action; eps_out is the kernel's own record of the eps it used
template <> struct PolicyTraits<AsvSacPolicy> : PolicyDefaults {
  static constexpr int kPol = kPolSac;
  static constexpr size_t kHeadBytes = sizeof(sactile::SacHeadLds);
  static int eps_rows(const AsvSacPolicy* pi) { return pi->deterministic != 0 ? 2 : 1; }
  static int checks(const char* who, const AsvStepCtl* ctl, const AsvSacPolicy* pi) {
    ENV_REQUIRE(ctl->is_continuous, "is_continuous must be 1 (SAC's actions are continuous)");
    if (int rc = mlp_images(who, pi->w.trunk, "null SAC actor image")) return rc;
    ENV_REQUIRE(pi->w.head != nullptr, "null pi->w.head");
    ENV_REQUIRE(pi->w.bhead != nullptr, "null pi->w.bhead");
    return 0;
  }
  static int act(const AsvSacPolicy* pi, const ActStep& s, void* stream) {
    AsvSacActIO io{};
    io.x = s.x;
    io.ldx = ASVRL_OBS_DIM;
    io.n = static_cast<int32_t>(s.n);
    io.a_out64 = s.act;
    io.eps_in = s.eps_zero;
    io.eps_out = s.eps_out;
    act_schedule(io, pi, s.step);
    return asvrl_sac_act(&pi->w, &io, stream);
  }
};

// IQN_Policy: the critic trunk's images (no MLP trunk), the padded head, the risk level. No window kernel: IQN's
// 150 KB image and 16 waves do not fit beside the env's carve. act_iqn with K = 32 taus per state, drawn in the kernel.
template <> struct PolicyTraits<AsvIqnPolicy> : PolicyDefaults {
  static constexpr bool kWindow = false, kActRecords = true;
  static int images(const char* who, const AsvStepCtl* ctl, const AsvIqnPolicy* pi) {
    ENV_REQUIRE(!ctl->is_continuous, "is_continuous must be 0 (IQN's actions are indices)");
    const AsvCriticWeights& w = pi->w;
    ENV_REQUIRE(w.wc_frag && w.w1_frag && w.w2_frag && w.bc && w.b1 && w.b2 && w.self_w && w.self_b && w.obj_w && w.obj_b,
                "null IQN image");
    ENV_REQUIRE(pi->head.wo_frag != nullptr, "null pi->head.wo_frag");
    ENV_REQUIRE(pi->head.bo != nullptr, "null pi->head.bo");
    ENV_REQUIRE(pi->head.n_actions >= 1 && pi->head.n_actions <= ASVRL_IQN_MAX_ACTIONS, "pi->head.n_actions must be in 1..32");
    return 0;
  }
  static int checks(const char* who, const AsvStepCtl* ctl, const AsvIqnPolicy* pi) {
    if (int rc = images(who, ctl, pi)) return rc;
    ENV_REQUIRE(pi->cvar > 0.f && pi->cvar <= 1.f, "pi->cvar must be in (0, 1]");
    return 0;
  }
  static AsvIqnIO act_io(const AsvIqnPolicy* pi, const ActStep& s) {
    AsvIqnIO io{};
    io.obs = s.x;
    io.ld_obs = ASVRL_OBS_DIM;
    io.B = static_cast<int32_t>(s.n);
    io.N = 32;
    act_schedule(io, pi, s.step);
    return io;
  }
  static AsvIqnActEx act_ex(const ActStep& s, float cvar) {
    AsvIqnActEx ex{};
    ex.cvar = cvar;
    ex.robots_per_env = s.robots_per_env;
    ex.step_add = s.step_add;
    ex.act_pair = s.act;
    ex.rec_row = s.rec_row;
    ex.env_mask = s.env_mask;
    return ex;
  }
  static int act(const AsvIqnPolicy* pi, const ActStep& s, void* stream) {
    const AsvIqnIO io = act_io(pi, s);
    const AsvIqnActEx ex = act_ex(s, pi->cvar);
    return asvrl_iqn_act_ex(&pi->w, &pi->head, &io, &ex, stream);
  }
};

// IQN_Policy under a per-robot risk level (asvrl_iqn_rollout_risk): the policy struct with the call's AsvIqnRisk
// beside it; every step's act launch is asvrl_iqn_act_risk (rows: the levels per robot slot, the same at every step;
// adaptive: from the row the robot acts on). The window always acts on observation rows.
struct IqnRiskPolicy : AsvIqnPolicy {
  const AsvIqnRisk* risk;
};
template <> struct PolicyTraits<IqnRiskPolicy> : PolicyDefaults {
  using Iqn = PolicyTraits<AsvIqnPolicy>;
  static constexpr bool kWindow = false, kActRecords = true;
  static int checks(const char* who, const AsvStepCtl* ctl, const IqnRiskPolicy* pi) {
    if (int rc = Iqn::images(who, ctl, pi)) return rc;
    if (const char* what = iqn_risk_problem(pi->risk, true)) return env_fail(who, what);
    ENV_REQUIRE(pi->cvar == 1.f, "pi->cvar must be 1 (the level comes from risk)");
    return 0;
  }
  static int act(const IqnRiskPolicy* pi, const ActStep& s, void* stream) {
    const AsvIqnIO io = Iqn::act_io(pi, s);
    const AsvIqnActEx ex = Iqn::act_ex(s, 1.f);
    AsvIqnRisk risk = *pi->risk;
    risk.cvar_out = nullptr;
    return asvrl_iqn_act_risk(&pi->w, &pi->head, &io, &ex, &risk, stream);
  }
};

// Rainbow_Policy: asvrl_rainbow_pack's forward images and the support. No window kernel: its tile is 4 MFMA waves per
// 32 rows with an LDS layout of its own.
template <> struct PolicyTraits<AsvRainbowPolicy> : PolicyDefaults {
  static constexpr bool kWindow = false, kActRecords = true;
  static int checks(const char* who, const AsvStepCtl* ctl, const AsvRainbowPolicy* pi) {
    ENV_REQUIRE(!ctl->is_continuous, "is_continuous must be 0 (Rainbow's actions are indices)");
    const AsvRainbowImg& w = pi->w;
    ENV_REQUIRE(w.enc && w.b_enc && w.v1 && w.a1 && w.v2 && w.a2 && w.vo && w.mo && w.ao && w.b_v1p && w.b_a1p &&
                    w.b_v2p && w.b_a2p && w.b_vop && w.b_mop && w.b_aop,
                "null Rainbow image");
    ENV_REQUIRE(pi->support != nullptr, "null pi->support");
    ENV_REQUIRE(pi->eps_total > 0.0 && pi->eps_fraction > 0.0, "pi->eps_total and pi->eps_fraction must be > 0");
    return 0;
  }
  static int act(const AsvRainbowPolicy* pi, const ActStep& s, void* stream) {
    AsvRainbowNetIO io{};
    io.x = s.x;
    io.ldx = ASVRL_OBS_DIM;
    io.N = static_cast<int32_t>(s.n);
    io.support = pi->support;
    act_schedule(io, pi, s.step);
    AsvRainbowActEx ex{};
    ex.robots_per_env = s.robots_per_env;
    ex.step_add = s.step_add;
    ex.act_pair = s.act;
    ex.rec_row = s.rec_row;
    ex.env_mask = s.env_mask;
    return asvrl_rainbow_net_act_ex(&pi->w, &io, &ex, stream);
  }
};

// The argument checks of the step and the rollout calls, in the order each call reports them (`who` names the call
// in the error text). roll: a rollout, which carries its actions / noise in ro (the single step's are the arguments
// here); reset: an _ar call, whatever ar points to. Pol other than NoPolicy: the closed loop under *pi.
template <class Pol>
static int env_checks(const char* who, bool roll, bool reset, const AsvParams* params, const AsvEnvState* state,
                      const double* actions, const double* noise, const AsvStepCtl* ctl, const AsvStepOut* out,
                      const AsvRollout* ro, const Pol* pi, const AsvAutoReset* ar, const AsvEnvLaunch* launch) {
  constexpr bool closed = !std::is_same_v<Pol, NoPolicy>;
  ENV_REQUIRE(params && state && ctl && out && (ro || !roll), "null argument");
  if (reset) {   // what the _ar calls refuse beyond their plain calls' checks
    ENV_REQUIRE(ar != nullptr, "null ar (the auto-reset description)");
    ENV_REQUIRE(!ro->hold_done, "ro->hold_done cannot be combined with the auto-reset");
    ENV_REQUIRE(ctl->trainer_deactivate && out->env_done != nullptr,
                "the auto-reset needs ctl->trainer_deactivate and last->env_done");
    ENV_REQUIRE(ctl->noise_mode == 1 || ctl->noise_mode == 2,
                "noise_mode 0 (recorded noise) cannot cover a sampled reset; Philox noise only (mode 1 or 2)");
    ENV_REQUIRE(closed || ar->obs_prev == nullptr || ar->obs_in != nullptr,
                "ar->obs_prev needs ar->obs_in (the rows in front of step 0)");
    ENV_REQUIRE(ar->cfg.num_robots >= 0 && ar->cfg.num_robots <= kResetMaxR && state->max_robots <= kResetMaxR,
                "ar->cfg.num_robots / max_robots beyond the reset sampler's 32");
    ENV_REQUIRE(ar->cfg.num_obs >= 0 && ar->cfg.num_obs <= kResetMaxO && state->max_obs <= kResetMaxO,
                "ar->cfg.num_obs / max_obs beyond the reset sampler's 32");
    ENV_REQUIRE(ar->cfg.num_cores >= 0 && ar->cfg.num_cores <= kMaxCores && state->max_cores <= kMaxCores,
                "ar->cfg.num_cores / max_cores beyond the reset sampler's 16");
    ENV_REQUIRE(ar->cfg.width > 4.0 && ar->cfg.height > 4.0, "ar->cfg map too small");
  }
  if (roll) {
    ENV_REQUIRE(ro->n_steps >= 1, "n_steps must be >= 1");
    if (!closed) ENV_REQUIRE(ro->actions != nullptr, "null actions");
  }
  if constexpr (closed) {
    ENV_REQUIRE(ro->actions == nullptr, "ro->actions must be null (the policy supplies the actions)");
    ENV_REQUIRE(pi != nullptr, "null policy");
    ENV_REQUIRE(pi->obs_in != nullptr, "null obs_in");
    if (int rc = PolicyTraits<Pol>::checks(who, ctl, pi)) return rc;
  }
  if (roll) {
    ENV_REQUIRE(ctl->do_dynamics, "do_dynamics must be 1");
    ENV_REQUIRE(!ro->hold_done || ctl->trainer_deactivate, "hold_done needs trainer_deactivate");
    ENV_REQUIRE(ctl->noise_mode != 0 || ro->noise != nullptr, "noise_mode 0 needs injected noise");
    ENV_REQUIRE(!(ro->hold_done || ro->env_done) || (ctl->trainer_deactivate && out->env_done),
                "hold_done and the env_done record need trainer_deactivate and out->env_done");
  }
  ENV_REQUIRE(state->max_robots >= 1 && state->max_robots <= kBlock, "max_robots must be in [1, 256]");
  ENV_REQUIRE(state->max_obs >= 0 && state->max_cores >= 0 && state->max_cores <= kMaxCoresStep,
              "bad max_obs/max_cores");
  ENV_REQUIRE(params->max_obj_num >= 0 && params->max_obj_num <= ASVRL_MAX_OBJ, "max_obj_num > 5");
  ENV_REQUIRE(params->N >= 1, "N < 1");
  ENV_REQUIRE(out->obs && out->obj_cnt && out->reward && out->done && out->info, "null output");
  if (!roll) {
    ENV_REQUIRE(ctl->noise_mode != 0 || noise != nullptr, "noise_mode 0 needs injected noise");
    ENV_REQUIRE(!ctl->do_dynamics || actions != nullptr, "actions required");
  }
  ENV_REQUIRE(state->rs && state->rflags && state->n_robots && state->n_obs && state->n_cores && state->ep_ts,
              "null state array");
  if (launch != nullptr && state->n_envs != 0) {
    ENV_REQUIRE(launch->layout >= 0 && launch->layout <= 2, "layout must be 0 (auto), 1 (pairs) or 2 (sweep)");
    ENV_REQUIRE(launch->block == 0 || launch->block == 64 || launch->block == 128 || launch->block == 256,
                "block must be 0, 64, 128 or 256");
    ENV_REQUIRE(launch->envs_per_block >= 0 && launch->max_groups >= 0, "negative envs_per_block / max_groups");
  }
  if constexpr (closed)
    ENV_REQUIRE(reinterpret_cast<uintptr_t>(pi->obs_in) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(out->obs) % 16 == 0 &&
                    (!reset || reinterpret_cast<uintptr_t>(ar->obs_prev) % 16 == 0),
                "observation rows must be 16-byte aligned");
  else if (reset)
    ENV_REQUIRE(ar->obs_prev == nullptr || (reinterpret_cast<uintptr_t>(ar->obs_in) % 16 == 0 &&
                                            reinterpret_cast<uintptr_t>(ar->obs_prev) % 16 == 0),
                "ar->obs_in / ar->obs_prev rows must be 16-byte aligned");
  return 0;
}

// The closed-loop launch's shape: 256-lane workgroups, one per CU (the Actor's weights fill most of its LDS), so
// enough envs per workgroup that the batch makes about one workgroup per CU (4096 envs x 5 robots: 16 envs, 256
// workgroups), never fewer than the open-loop shape's, and as many as the LDS left beside the weights holds.
// AsvEnvLaunch overrides block and envs_per_block. fits = false: the K-launch fallback.
struct PolicyLaunch {
  PairLaunch pl;
  size_t smem;   // dynamic: the pair carve + the observation rows and action pairs
  bool fits;
};
// head_bytes: static LDS beside the Actor's images (SAC's f32 head).
static PolicyLaunch policy_launch(int R, int O, int n_envs, int blk_req, int epb_req, int vm_bytes, bool ar = false,
                                  size_t head_bytes = 0) {
  constexpr size_t kLdsBytes = 160 * 1024;
  constexpr size_t kLdsStatic = 1024;   // room for the workgroup-vote scratch (__syncthreads_or) and alignment
  static_assert(sizeof(atile::ActorLds) + sizeof(sactile::SacHeadLds) + kLdsStatic < kLdsBytes,
                "the actor's images, the SAC head and the vote scratch leave room for a carve in one CU's LDS");
  constexpr int kCus = 256;
  auto total = [&](const PairLaunch& l) {
    const size_t rows = policy_rows_offset(l.smem) + static_cast<size_t>(l.epb) * R * (ASVRL_OBS_DIM * sizeof(float) + 2 * sizeof(double));
    return ar ? policy_rows_offset(rows) + autoreset_lds(l.blk, l.epb) : rows;   // (the auto-reset's LDS behind the rows)
  };
  PolicyLaunch L;
  int blk = (blk_req == 64 || blk_req == 128) ? blk_req : 256;
  if (R > blk) blk = 256;
  int epb = epb_req;
  if (epb <= 0) {
    const int base = pair_launch(R, O, n_envs, blk, 0, vm_bytes).epb, per_cu = (n_envs + kCus - 1) / kCus;
    epb = per_cu > base ? per_cu : base;
  }
  for (;;) {
    L.pl = pair_launch(R, O, n_envs, blk, epb, vm_bytes);   // (at most blk / R envs)
    L.smem = total(L.pl);
    L.fits = sizeof(atile::ActorLds) + head_bytes + kLdsStatic + L.smem <= kLdsBytes;
    if (L.fits || epb_req > 0 || L.pl.epb <= 1) break;
    epb = L.pl.epb - 1;
  }
  return L;
}

// The resolved launch of one call.
struct EnvPlan {
  int nm;              // the kernels' noise argument: 0 recorded rows, 1 Philox, 2 Philox with f32 radius draws
  bool per_robot;      // per-robot parameters: the sweep layout only
  bool fused;          // the pair-parallel kernel is taken; false: the sweep step / the K-launch fallback
  PairLaunch pl;       // (fused only, as everything below)
  size_t smem;         // dynamic LDS: the pair carve, the policy rows (closed loop), the auto-reset's LDS
  int ar_off;          // where the auto-reset's LDS starts in it
  int groups, chunk;   // workgroups in all and per launch (AsvEnvLaunch max_groups)
};
// The open loop takes the pair layout where its carve fits 150 KB, and refuses an explicit layout 1 that cannot be
// had; the closed loop takes it where policy_launch fits the carve beside the Actor (and head_bytes: SAC's head), and
// falls back otherwise.
static int env_plan(const char* who, const AsvEnvState* state, const AsvStepCtl* ctl, const AsvEnvLaunch* launch,
                    bool closed, bool ar, EnvPlan* plan, size_t head_bytes = 0) {
  const AsvEnvLaunch lz{};
  const AsvEnvLaunch& lc = launch != nullptr ? *launch : lz;
  EnvPlan P{};
  P.nm = ctl->noise_mode == 0 ? 0 : (ctl->noise_mode == 1 ? 1 : 2);
  P.per_robot = state->robot_params != nullptr;
  const int vm_bytes = P.nm == 2 ? 4 : 8;
  if (!closed) {
    P.pl = pair_launch(state->max_robots, state->max_obs, state->n_envs, lc.block, lc.envs_per_block, vm_bytes);
    P.smem = P.pl.smem;
    if (ar) {
      P.ar_off = static_cast<int>(policy_rows_offset(P.pl.smem));
      P.smem = P.ar_off + autoreset_lds(P.pl.blk, P.pl.epb);
    }
    ENV_REQUIRE(lc.layout != 1 || P.smem <= 150 * 1024, "the pair layout's LDS does not fit");
    ENV_REQUIRE(lc.layout != 1 || !P.per_robot, "per-robot parameters take the sweep layout (2)");
    P.fused = lc.layout != 2 && !P.per_robot && P.smem <= 150 * 1024;
  } else if (lc.layout != 2 && !P.per_robot) {
    const PolicyLaunch L = policy_launch(state->max_robots, state->max_obs, state->n_envs, lc.block, lc.envs_per_block,
                                         vm_bytes, ar, head_bytes);
    P.pl = L.pl;
    P.smem = L.smem;
    if (ar) P.ar_off = static_cast<int>(L.smem - autoreset_lds(L.pl.blk, L.pl.epb));
    P.fused = L.fits;
  }
  if (P.fused) {
    P.groups = (state->n_envs + P.pl.epb - 1) / P.pl.epb;
    P.chunk = lc.max_groups > 0 && lc.max_groups < P.groups ? lc.max_groups : P.groups;
  }
  *plan = P;
  return 0;
}

// The kernel of an argument struct, and the PairsArgs in it. The auto-reset windows exist for Philox noise only.
template <int B, int NM> static auto kernel_of(const PairsArgs&) { return &env_pairs_kernel<B, NM>; }
template <int B, int NM, class Pol, bool AR> static auto kernel_of(const WindowArgs<Pol, AR>&) {
  if constexpr (std::is_same_v<Pol, NoPolicy>)
    return &env_rollout_kernel<B, NM, AR>;
  else
    return &env_policy_rollout_kernel<B, NM, PolicyTraits<Pol>::kPol, AR>;
}
template <class Args> constexpr bool kPhiloxOnly = false;
template <class Pol> constexpr bool kPhiloxOnly<WindowArgs<Pol, true>> = true;
static PairsArgs& pairs_of(PairsArgs& a) { return a; }
template <class Args> static PairsArgs& pairs_of(Args& a) { return a.k; }

template <int B, class Args>
static auto kernel_for_noise(int nm, const Args& a) -> void (*)(Args) {
  if constexpr (!kPhiloxOnly<Args>) {
    if (nm == 0) return kernel_of<B, 0>(a);
  }
  return nm == 1 ? kernel_of<B, 1>(a) : kernel_of<B, 2>(a);
}
// The pair-parallel launch of the step's kernel or a window's: P.groups workgroups in launches of at most P.chunk,
// each told its first group.
template <class Args>
static int launch_groups(const char* who, const EnvPlan& P, Args a, hipStream_t st) {
  void (*const kern)(Args) = P.pl.blk == 64    ? kernel_for_noise<64>(P.nm, a)
                             : P.pl.blk == 128 ? kernel_for_noise<128>(P.nm, a)
                                               : kernel_for_noise<256>(P.nm, a);
  for (int g0 = 0; g0 < P.groups; g0 += P.chunk) {
    pairs_of(a).group0 = g0;
    hipLaunchKernelGGL(kern, dim3(P.groups - g0 < P.chunk ? P.groups - g0 : P.chunk), dim3(P.pl.blk), P.smem, st, a);
  }
  return check_launch(who);
}

extern "C" int asvrl_env_step_ex(const AsvParams* params, const AsvEnvState* state, const double* actions,
                                 const double* noise, const AsvStepCtl* ctl, const AsvStepOut* out,
                                 const AsvEnvLaunch* launch, void* stream) {
  const char* who = "asvrl_env_step";
  if (int rc = env_checks(who, false, false, params, state, actions, noise, ctl, out, nullptr, kOpenLoop, nullptr,
                          launch))
    return rc;
  if (state->n_envs == 0) return 0;
  EnvPlan P;
  if (int rc = env_plan(who, state, ctl, launch, false, false, &P)) return rc;
  if (P.fused)
    return launch_groups(who, P, PairsArgs{*params, *state, *ctl, *out, actions, noise, P.pl.epb, 0}, as_stream(stream));
  const int blk = step_block(state->max_robots);
  const int epb = blk / state->max_robots;
  const int grid = (state->n_envs + epb - 1) / epb;
  const size_t smem = env_sweep_smem(state->max_robots, state->max_obs);
  ASVRL_REQUIRE(smem <= 160 * 1024, "asvrl_env_step: max_obs too large for LDS");
  auto sweep = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(blk), smem, as_stream(stream), *params, *state, actions, noise, *ctl,
                       *out);
  };
  if (blk == 64)
    P.per_robot ? sweep(env_sweep_kernel<64, true>) : sweep(env_sweep_kernel<64, false>);
  else
    P.per_robot ? sweep(env_sweep_kernel<256, true>) : sweep(env_sweep_kernel<256, false>);
  return check_launch(who);
}

extern "C" int asvrl_env_step(const AsvParams* params, const AsvEnvState* state, const double* actions,
                              const double* noise, const AsvStepCtl* ctl, const AsvStepOut* out, void* stream) {
  return asvrl_env_step_ex(params, state, actions, noise, ctl, out, nullptr, stream);
}

// The K-launch form of the rollout calls (per-robot parameters, layout 2, a carve that does not fit; always, for a
// policy without a window kernel). Per step: the act launch (closed loop: PolicyTraits<Pol>::act, between the
// step-count and the record-copy launch unless it does both itself), the obs_prev row (auto-reset), the single step
// and its record launch; then, for the auto-reset, the reset mask and counts and the reset of the ended envs with
// their observation (asvrl_env_reset_observe, or the two launches where that call does not apply). NoPolicy: the open
// loop, the actions out of ro. ar null: a plain call, which alone can hold ended envs (hold_done: env_checks refuses
// it with ar).
template <class Pol>
static int rollout_fallback(const char* who, const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                            const AsvStepOut* out, const AsvRollout* ro, const Pol* pi, const AsvAutoReset* ar,
                            const AsvEnvLaunch* launch, void* stream) {
  using T = PolicyTraits<Pol>;
  constexpr bool closed = !std::is_same_v<Pol, NoPolicy>;
  hipStream_t st = as_stream(stream);
  const int E = state->n_envs, R = state->max_robots;
  const size_t NT = static_cast<size_t>(E) * R;
  const size_t noise_row = NT * (static_cast<size_t>(state->max_obs) + R) * 5;
  const unsigned egrid = (static_cast<unsigned>(E) + kBlock - 1) / kBlock;
  const unsigned agrid = (static_cast<unsigned>(NT) + kBlock - 1) / kBlock;
  const unsigned qgrid = (static_cast<unsigned>(NT) * (ASVRL_OBS_DIM / 4) + kBlock - 1) / kBlock;
  // stream-ordered scratch: the actions [NT][2] f64 and the act launch's step count (closed loop), then the policy's
  // eps arrays [NT][2] f32 (SAC: eps_out and, when deterministic, the zero eps_in), then the reset mask [E]
  // (auto-reset); hold_done's mask [E] is an allocation of its own
  const size_t pol_bytes = closed ? sizeof(double) * 2 * NT + sizeof(int64_t) : 0;
  const size_t eps_bytes = sizeof(float) * 2 * NT;
  const int eps_rows = T::eps_rows(pi);
  const size_t act_bytes = pol_bytes + eps_bytes * eps_rows;
  const size_t scratch_bytes = act_bytes + (ar != nullptr ? E : 0);
  unsigned char* scratch = nullptr;
  if (scratch_bytes != 0 && hipMallocAsync(reinterpret_cast<void**>(&scratch), scratch_bytes, st) != hipSuccess)
    return check_launch(who);
  double* act = reinterpret_cast<double*>(scratch);
  int64_t* step = closed ? reinterpret_cast<int64_t*>(act + 2 * NT) : nullptr;
  uint8_t* rmask = ar != nullptr ? scratch + act_bytes : nullptr;
  float* eps_out = eps_rows >= 1 ? reinterpret_cast<float*>(scratch + pol_bytes) : nullptr;
  float* eps_zero = eps_rows >= 2 ? eps_out + 2 * NT : nullptr;
  int rc = 0;
  if (eps_zero != nullptr && hipMemsetAsync(eps_zero, 0, eps_bytes, st) != hipSuccess) rc = check_launch(who);
  uint8_t* hold_mask = nullptr;
  if (ro->hold_done) {
    if (hipMallocAsync(reinterpret_cast<void**>(&hold_mask), E, st) != hipSuccess)
      rc = check_launch(who);
    else if (ctl->env_mask != nullptr)
      (void)hipMemcpyAsync(hold_mask, ctl->env_mask, E, hipMemcpyDeviceToDevice, st);
    else
      (void)hipMemsetAsync(hold_mask, 1, E, st);
  }
  bool one_launch = false;   // the auto-reset's reset and observation in one launch
  if (ar != nullptr) {
    const PairLaunch one = pair_launch(R, state->max_obs, E, kWave, 1, ctl->noise_mode == 2 ? 4 : 8);
    one_launch = state->robot_params == nullptr && one.blk == kWave && one.epb == 1 && one.smem <= 60 * 1024;
  }
  AsvStepOut oo = *out;   // the observation pass's outputs: no episode bookkeeping
  oo.env_done = nullptr;
  oo.stats = nullptr;
  const float* obs_first = ar != nullptr ? ar->obs_in : nullptr;
  if constexpr (closed) obs_first = pi->obs_in;
  for (int t = 0; t < ro->n_steps && rc == 0; ++t) {
    AsvStepCtl c = *ctl;
    c.counter = ctl->counter + static_cast<uint64_t>(t);
    if (hold_mask != nullptr) c.env_mask = hold_mask;
    const float* obs_t = t == 0 ? obs_first : out->obs;   // the observation the step before (or its reset) wrote
    const double* actions = act;
    if constexpr (closed) {
      double* rec_row = pi->actions != nullptr ? pi->actions + static_cast<size_t>(t) * 2 * NT : nullptr;
      if constexpr (T::kActRecords) {
        // one launch: the act at step *step_dev + t, the step's pairs and the record row under the step's mask
        rc = T::act(pi, ActStep{obs_t, NT, act, pi->step_dev, t, R, rec_row, c.env_mask, eps_out, eps_zero}, stream);
      } else {
        hipLaunchKernelGGL(policy_step_count_kernel, dim3(1), dim3(1), 0, st, pi->step_dev, step, t);
        rc = T::act(pi, ActStep{obs_t, NT, act, step, 0, R, nullptr, nullptr, eps_out, eps_zero}, stream);
        if (rc == 0 && rec_row != nullptr)
          hipLaunchKernelGGL(policy_actions_kernel, dim3(agrid), dim3(kBlock), 0, st, act, rec_row, c.env_mask, E, R);
      }
    } else {
      actions = ro->actions + static_cast<size_t>(t) * 2 * NT;
    }
    if (rc == 0 && ar != nullptr && ar->obs_prev != nullptr)
      hipLaunchKernelGGL(autoreset_obs_prev_kernel, dim3(qgrid), dim3(kBlock), 0, st, obs_t,
                         ar->obs_prev + static_cast<size_t>(t) * NT * ASVRL_OBS_DIM, c.env_mask, E, R);
    // recorded noise rows go to the plain calls only: the auto-reset is Philox noise throughout (env_checks)
    const double* noise = ar == nullptr && ro->noise != nullptr ? ro->noise + static_cast<size_t>(t) * noise_row : nullptr;
    if (rc == 0) rc = asvrl_env_step_ex(params, state, actions, noise, &c, out, launch, stream);
    if (rc != 0) break;
    hipLaunchKernelGGL(rollout_record_kernel, dim3(egrid), dim3(kBlock), 0, st, *state, *out, *ro, t, c.env_mask,
                       hold_mask);
    if (ar != nullptr)
      hipLaunchKernelGGL(autoreset_mask_kernel, dim3(egrid), dim3(kBlock), 0, st, out->env_done, c.env_mask, out->obj_cnt,
                         E, R, rmask, ar->resets, ar->pushed != nullptr ? ar->pushed + t : nullptr);
    rc = check_launch(who);
    if (rc != 0 || ar == nullptr) continue;
    AsvStepCtl co{};
    co.is_continuous = ctl->is_continuous;
    co.noise_mode = ctl->noise_mode;
    co.seed = ctl->seed;
    co.counter = ar->obs_counter + static_cast<uint64_t>(t);
    co.counter_dev = ctl->counter_dev;
    co.env_mask = rmask;
    const uint64_t rctr = ar->reset_counter + static_cast<uint64_t>(t);
    if (one_launch) {
      rc = asvrl_env_reset_observe(params, state, &ar->cfg, rmask, ctl->seed, rctr, ctl->counter_dev, &co, &oo, stream);
    } else {
      rc = asvrl_env_reset(params, state, &ar->cfg, rmask, ctl->seed, rctr, ctl->counter_dev, stream);
      if (rc == 0) rc = asvrl_env_step_ex(params, state, nullptr, nullptr, &co, &oo, launch, stream);
    }
  }
  if (hold_mask != nullptr) (void)hipFreeAsync(hold_mask, st);
  if (scratch != nullptr) (void)hipFreeAsync(scratch, st);
  return rc;
}

// A rollout call: check, plan, zero the counts the window adds to, then the one launch or the fallback. AR: an _ar
// call, the auto-reset described by ar (Philox noise only: no recorded rows); a plain call passes ar null. Pol other
// than NoPolicy: the closed loop under *pi (ro->actions is null then).
template <bool AR, class Pol>
static int rollout_call(const char* who, const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                        const AsvStepOut* out, const AsvRollout* ro, const Pol* pi, const AsvAutoReset* ar,
                        const AsvEnvLaunch* launch, void* stream) {
  using T = PolicyTraits<Pol>;
  if (int rc = env_checks(who, true, AR, params, state, nullptr, nullptr, ctl, out, ro, pi, ar, launch)) return rc;
  if (state->n_envs == 0) return 0;
  EnvPlan P{};
  if constexpr (T::kWindow) {
    if (int rc = env_plan(who, state, ctl, launch, !std::is_same_v<Pol, NoPolicy>, AR, &P, T::kHeadBytes)) return rc;
  }
  hipStream_t st = as_stream(stream);
  if (ro->steps_run != nullptr && hipMemsetAsync(ro->steps_run, 0, sizeof(int32_t) * state->n_envs, st) != hipSuccess)
    return check_launch(who);
  if (AR && ar->resets != nullptr &&
      hipMemsetAsync(ar->resets, 0, sizeof(int32_t) * state->n_envs, st) != hipSuccess)
    return check_launch(who);
  if constexpr (T::kWindow) {
    if (P.fused) {
      WindowArgs<Pol, AR> a{
          PairsArgs{*params, *state, *ctl, *out, ro->actions, AR ? nullptr : ro->noise, P.pl.epb, 0}, *ro};
      if constexpr (!std::is_same_v<Pol, NoPolicy>) a.pi = *pi;
      if constexpr (AR) {
        a.ar = *ar;
        a.ar_off = P.ar_off;
      }
      return launch_groups(who, P, a, st);
    }
  }
  return rollout_fallback(who, params, state, ctl, out, ro, pi, ar, launch, stream);
}

extern "C" int asvrl_env_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                 const AsvStepOut* out, const AsvRollout* ro, const AsvEnvLaunch* launch,
                                 void* stream) {
  return rollout_call<false>("asvrl_env_rollout", params, state, ctl, out, ro, kOpenLoop, nullptr, launch, stream);
}

extern "C" int asvrl_policy_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                    const AsvStepOut* out, const AsvRollout* ro, const AsvPolicy* pi,
                                    const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<false>("asvrl_policy_rollout", params, state, ctl, out, ro, pi, nullptr, launch, stream);
}

extern "C" int64_t asvrl_policy_struct_size(void) { return sizeof(AsvPolicy); }

extern "C" int asvrl_env_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                    const AsvStepOut* out, const AsvRollout* ro, const AsvAutoReset* ar,
                                    const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<true>("asvrl_env_rollout_ar", params, state, ctl, out, ro, kOpenLoop, ar, launch, stream);
}

extern "C" int asvrl_policy_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                       const AsvStepOut* out, const AsvRollout* ro, const AsvPolicy* pi,
                                       const AsvAutoReset* ar, const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<true>("asvrl_policy_rollout_ar", params, state, ctl, out, ro, pi, ar, launch, stream);
}

extern "C" int asvrl_dqn_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                 const AsvStepOut* out, const AsvRollout* ro, const AsvDqnPolicy* pi,
                                 const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<false>("asvrl_dqn_rollout", params, state, ctl, out, ro, pi, nullptr, launch, stream);
}

extern "C" int asvrl_dqn_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                    const AsvStepOut* out, const AsvRollout* ro, const AsvDqnPolicy* pi,
                                    const AsvAutoReset* ar, const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<true>("asvrl_dqn_rollout_ar", params, state, ctl, out, ro, pi, ar, launch, stream);
}

extern "C" int64_t asvrl_dqn_policy_struct_size(void) { return sizeof(AsvDqnPolicy); }

extern "C" int asvrl_sac_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                 const AsvStepOut* out, const AsvRollout* ro, const AsvSacPolicy* pi,
                                 const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<false>("asvrl_sac_rollout", params, state, ctl, out, ro, pi, nullptr, launch, stream);
}

extern "C" int asvrl_sac_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                    const AsvStepOut* out, const AsvRollout* ro, const AsvSacPolicy* pi,
                                    const AsvAutoReset* ar, const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<true>("asvrl_sac_rollout_ar", params, state, ctl, out, ro, pi, ar, launch, stream);
}

extern "C" int64_t asvrl_sac_policy_struct_size(void) { return sizeof(AsvSacPolicy); }

extern "C" int asvrl_iqn_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                 const AsvStepOut* out, const AsvRollout* ro, const AsvIqnPolicy* pi,
                                 const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<false>("asvrl_iqn_rollout", params, state, ctl, out, ro, pi, nullptr, launch, stream);
}

extern "C" int asvrl_iqn_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                    const AsvStepOut* out, const AsvRollout* ro, const AsvIqnPolicy* pi,
                                    const AsvAutoReset* ar, const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<true>("asvrl_iqn_rollout_ar", params, state, ctl, out, ro, pi, ar, launch, stream);
}

extern "C" int64_t asvrl_iqn_policy_struct_size(void) { return sizeof(AsvIqnPolicy); }

// the policy of a _risk call: *pi with the risk beside it (a null pi stays null: env_checks names it)
static const IqnRiskPolicy* risk_policy(IqnRiskPolicy& p, const AsvIqnPolicy* pi, const AsvIqnRisk* risk) {
  if (pi == nullptr) return nullptr;
  static_cast<AsvIqnPolicy&>(p) = *pi;
  p.risk = risk;
  return &p;
}

extern "C" int asvrl_iqn_rollout_risk(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                      const AsvStepOut* out, const AsvRollout* ro, const AsvIqnPolicy* pi,
                                      const AsvIqnRisk* risk, const AsvEnvLaunch* launch, void* stream) {
  IqnRiskPolicy p{};
  return rollout_call<false>("asvrl_iqn_rollout_risk", params, state, ctl, out, ro, risk_policy(p, pi, risk), nullptr,
                             launch, stream);
}

extern "C" int asvrl_iqn_rollout_risk_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                         const AsvStepOut* out, const AsvRollout* ro, const AsvIqnPolicy* pi,
                                         const AsvIqnRisk* risk, const AsvAutoReset* ar, const AsvEnvLaunch* launch,
                                         void* stream) {
  IqnRiskPolicy p{};
  return rollout_call<true>("asvrl_iqn_rollout_risk_ar", params, state, ctl, out, ro, risk_policy(p, pi, risk), ar,
                            launch, stream);
}

extern "C" int asvrl_rainbow_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                     const AsvStepOut* out, const AsvRollout* ro, const AsvRainbowPolicy* pi,
                                     const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<false>("asvrl_rainbow_rollout", params, state, ctl, out, ro, pi, nullptr, launch, stream);
}

extern "C" int asvrl_rainbow_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                                        const AsvStepOut* out, const AsvRollout* ro, const AsvRainbowPolicy* pi,
                                        const AsvAutoReset* ar, const AsvEnvLaunch* launch, void* stream) {
  return rollout_call<true>("asvrl_rainbow_rollout_ar", params, state, ctl, out, ro, pi, ar, launch, stream);
}

extern "C" int64_t asvrl_rainbow_policy_struct_size(void) { return sizeof(AsvRainbowPolicy); }

extern "C" int64_t asvrl_autoreset_struct_size(void) { return sizeof(AsvAutoReset); }

extern "C" int asvrl_env_reset(const AsvParams* params, const AsvEnvState* state, const AsvResetCfg* cfg,
                               const uint8_t* env_mask, uint64_t seed, uint64_t counter,
                               const uint64_t* counter_dev, void* stream) {
  ASVRL_REQUIRE(params && state && cfg, "asvrl_env_reset: null argument");
  ASVRL_REQUIRE(state->max_cores <= kMaxCores, "asvrl_env_reset: max_cores > 16");
  ASVRL_REQUIRE(state->max_robots <= kResetMaxR && state->max_obs <= kResetMaxO,
                "asvrl_env_reset: max_robots and max_obs must be <= 32");
  ASVRL_REQUIRE(cfg->width > 4.0 && cfg->height > 4.0, "asvrl_env_reset: map too small");
  if (state->n_envs == 0) return 0;
  const int grid = (state->n_envs + kResetWaves - 1) / kResetWaves;
  hipLaunchKernelGGL(env_reset_kernel, dim3(grid), dim3(kResetWaves * kWave), 0, as_stream(stream), *params, *state,
                     *cfg, env_mask, seed, counter, counter_dev);
  return check_launch("asvrl_env_reset");
}

extern "C" int asvrl_env_reset_observe(const AsvParams* params, const AsvEnvState* state, const AsvResetCfg* cfg,
                                       const uint8_t* env_mask, uint64_t seed, uint64_t counter,
                                       const uint64_t* counter_dev, const AsvStepCtl* ctl, const AsvStepOut* out,
                                       void* stream) {
  ASVRL_REQUIRE(params && state && cfg && ctl && out && env_mask, "asvrl_env_reset_observe: null argument");
  ASVRL_REQUIRE(state->max_cores <= kMaxCores, "asvrl_env_reset_observe: max_cores > 16");
  ASVRL_REQUIRE(state->max_robots <= kResetMaxR && state->max_obs <= kResetMaxO,
                "asvrl_env_reset_observe: max_robots and max_obs must be <= 32");
  ASVRL_REQUIRE(cfg->width > 4.0 && cfg->height > 4.0, "asvrl_env_reset_observe: map too small");
  ASVRL_REQUIRE(state->robot_params == nullptr, "asvrl_env_reset_observe: per-robot parameters take the two-launch path");
  ASVRL_REQUIRE(!ctl->do_dynamics && ctl->env_mask == env_mask, "asvrl_env_reset_observe: ctl must be the masked "
                "observation pass (do_dynamics = 0, env_mask = the reset mask)");
  ASVRL_REQUIRE(ctl->noise_mode == 1 || ctl->noise_mode == 2, "asvrl_env_reset_observe: Philox noise only (mode 1 or 2)");
  ASVRL_REQUIRE(out->obs && out->obj_cnt && out->reward && out->done && out->info,
                "asvrl_env_reset_observe: null output");
  if (state->n_envs == 0) return 0;
  const PairLaunch pl = pair_launch(state->max_robots, state->max_obs, state->n_envs, kWave, 1,
                                    ctl->noise_mode == 2 ? 4 : 8);
  ASVRL_REQUIRE(pl.blk == kWave && pl.epb == 1 && pl.smem <= 60 * 1024, "asvrl_env_reset_observe: env too large");
  auto go = [&](auto kern) {
    const ResetObsArgs a{PairsArgs{*params, *state, *ctl, *out, nullptr, nullptr, 1, 0}, *cfg, env_mask, seed, counter,
                         counter_dev};
    hipLaunchKernelGGL(kern, dim3(state->n_envs), dim3(kWave), pl.smem, as_stream(stream), a);
  };
  ctl->noise_mode == 2 ? go(env_reset_observe_kernel<2>) : go(env_reset_observe_kernel<1>);
  return check_launch("asvrl_env_reset_observe");
}

extern "C" int asvrl_current_field(const double* cores, int32_t n_cores, double core_r, const double* xy,
                                   int32_t n, double* out, void* stream) {
  ASVRL_REQUIRE(xy && out && (n_cores == 0 || cores), "asvrl_current_field: null argument");
  ASVRL_REQUIRE(n_cores >= 0 && n_cores <= kMaxCoresStep, "asvrl_current_field: n_cores > 4096");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(current_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, as_stream(stream), cores,
                     n_cores, core_r, xy, n, out);
  return check_launch("asvrl_current_field");
}
