/* asvrl.h -- C ABI of libasvrl.so, the MI355X (gfx950) kernels behind the rfarl training
 * hot path: the vectorised ASV marine-env step and the distributional Bellman update.
 *
 * The reference (pszenher/Distributional_RL_Decision_and_Control, rfarl/) is pure Python
 * and has no FFI; each entry point below replaces the Python function cited next to it
 * (paths relative to /root/reference/rfarl/rfarl/). The Python surfaces that call these
 * (MarineNavEnv3, Agent, Trainer) live in distributional_rl_decision_and_control_amd/ and
 * bind this header through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every pointer argument is a DEVICE pointer unless its comment says "host".
 *    The caller owns all memory (allocated as torch tensors); the library keeps no state.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream). All work is
 *    stream-ordered; no entry point synchronises the device.
 *  - Return value: 0 on success, nonzero on a bad argument or launch failure, with a
 *    thread-local message from asvrl_last_error(). No C++ exception crosses the ABI.
 *  - Two builds export this same header: libasvrl.so, whose learner kernels take bf16 MFMA
 *    operands (weight images, saved activations) with f32 accumulation, and libasvrl_f32.so,
 *    the same sources with every such operand f32 (the parity build). "bf16" in the comments
 *    below means the operand element type: f32 in libasvrl_f32.so (asvrl_operand_bytes()).
 */
#ifndef ASVRL_H
#define ASVRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASVRL_ABI_VERSION 29

#define ASVRL_SELF_DIM 7   /* wamv.py:443-453 self observation */
#define ASVRL_OBJ_DIM 5    /* wamv.py:481,508 [px, py, vx, vy, r] */
#define ASVRL_MAX_OBJ 5    /* wamv.py:14 max_obj_num */
#define ASVRL_OBS_DIM 40   /* packed f32 obs row: self 7 | objects 5x5 | mask 5 | pad 3
                              (= replay_buffer.py:51-69 state_batch, padded to 16 B) */
#define ASVRL_TR_DIM 88    /* replay row: obs 40 | next obs 40 | action 2 | reward | done | pad 4 */
#define ASVRL_PER_DIM 48   /* prioritised replay slot: obs 40 | action | reward | nonterminal | timestep (i32) | pad 4 */

/* Robot state fields, field-major SoA: rs[f * (n_envs * max_robots) + e * max_robots + i] */
enum AsvRobotField {
  ASVRL_F_X = 0, ASVRL_F_Y, ASVRL_F_THETA,           /* wamv.py:92-94 */
  ASVRL_F_VR0, ASVRL_F_VR1, ASVRL_F_VR2,               /* velocity_r (wamv.py:95) */
  ASVRL_F_V0, ASVRL_F_V1, ASVRL_F_V2,                  /* velocity, one substep stale (:96) */
  ASVRL_F_TL, ASVRL_F_TR, ASVRL_F_LP, ASVRL_F_RP,      /* thrusts, thruster angles (:98-101) */
  ASVRL_F_GX, ASVRL_F_GY,                              /* goal (:129) */
  ASVRL_F_PHI,                                         /* COLREGs turn angle (:396) */
  ASVRL_F_RET,                                         /* discounted episode return (trainer.py:161) */
  ASVRL_NUM_FIELDS
};

/* Robot flag bits (u8 per robot) */
#define ASVRL_FLAG_DEACTIVATED 1u  /* wamv.py:132, written by trainer.py:168-170 */
#define ASVRL_FLAG_COLLISION 2u    /* wamv.py:130 */
#define ASVRL_FLAG_REACH_GOAL 4u   /* wamv.py:131 */
#define ASVRL_FLAG_COLREGS 8u      /* wamv.py:517-521 apply_COLREGs */

/* info codes of env.step (env.py:291-328) */
#define ASVRL_INFO_NORMAL 0
#define ASVRL_INFO_TOO_LONG 1
#define ASVRL_INFO_COLLISION 2
#define ASVRL_INFO_REACH_GOAL 3
#define ASVRL_INFO_DEACT_COLLISION 4
#define ASVRL_INFO_DEACT_GOAL 5
#define ASVRL_INFO_ABSENT 255      /* slot beyond the env's robot count */

/* Vehicle, perception and reward parameters (wamv.py:45-125, env.py:33-54). Passed by
 * value to the kernels; one set per env batch. */
typedef struct AsvParams {
  double dt;                 /* wamv.py:46 */
  int32_t N;                 /* wamv.py:47 substeps per action */
  int32_t episode_limit;     /* env.py:312 */
  double length, width;      /* wamv.py:51-52 */
  double r;                  /* collision radius = detect_r (wamv.py:53-54) */
  double goal_dis;           /* wamv.py:79 */
  double min_thrust, max_thrust; /* wamv.py:84-85 */
  double m, Izz;             /* wamv.py:103-104 */
  double xDotU, yDotV, yDotR, nDotR, nDotV, xU, xUU, yV, yVV, yR, yRV, yVR, yRR, nR, nRR, nV,
      nVV, nRV, nVR;         /* wamv.py:107-125 */
  double P[9];               /* inv(A^T A) A^T, A = M_RB + M_A (wamv.py:267-271), row-major,
                                computed on the host with the reference's numpy expression */
  double left_thrust_change[5], right_thrust_change[5]; /* wamv.py:86-88 discrete grid */
  double range, angle;       /* wamv.py:12-13 */
  double pos_std, vel_std, r_kappa, r_mean_ratio; /* wamv.py:22-25 */
  int32_t max_obj_num;       /* wamv.py:14 (<= ASVRL_MAX_OBJ) */
  int32_t _pad0;
  double timestep_penalty, COLREGs_penalty, collision_penalty, goal_reward; /* env.py:47-50 */
  double core_r;             /* env.py:35 vortex core radius */
} AsvParams;

/* A batch of E envs, resident in HBM. All arrays are caller-owned device memory. */
typedef struct AsvEnvState {
  int32_t n_envs, max_robots, max_obs, max_cores;
  double* rs;        /* [ASVRL_NUM_FIELDS][n_envs * max_robots] robot state (field-major SoA) */
  uint8_t* rflags;   /* [n_envs * max_robots] ASVRL_FLAG_* */
  int32_t* n_robots; /* [n_envs] robots placed by reset (<= max_robots; env.py:106-120 may place fewer) */
  int32_t* n_obs;    /* [n_envs] */
  int32_t* n_cores;  /* [n_envs] */
  int32_t* ep_ts;    /* [n_envs] episode_timesteps (env.py:64) */
  double* obstacles; /* [n_envs][max_obs][3] x, y, r (env.py:16-22) */
  double* cores;     /* [n_envs][max_cores][4] x, y, clockwise, Gamma (env.py:7-14) */
  const AsvParams* robot_params; /* optional [n_envs * max_robots]: each robot's own vehicle and
                                    perception parameters (reset_with_eval_config, env.py:553-607);
                                    NULL: `params` for every robot. The env-level members (episode
                                    limit, rewards, core radius) always come from `params`. Taken by the
                                    per-robot sweep layout (asvrl_env_step chooses it; layout 1 fails) */
} AsvEnvState;

/* Per-call control of asvrl_env_step. */
typedef struct AsvStepCtl {
  int32_t is_continuous;      /* env.step is_continuous_action (env.py:240) */
  int32_t do_dynamics;        /* 0: observation only (reset's get_observations, env.py:164) */
  int32_t trainer_deactivate; /* 1: apply trainer.py:157-172 in-kernel (deactivate on flags,
                                 episode-end test, discounted return) */
  int32_t noise_mode;         /* 0: injected draws (noise != NULL, parity with the reference's
                                 per-robot RandomState); 1: Philox-4x32-10 in registers, f64
                                 Box-Muller / von Mises; 2: Philox, f32 draws on the hardware
                                 transcendentals (the training path) */
  uint64_t seed, counter;     /* Philox key / per-step counter (noise_mode 1, 2) */
  const uint64_t* counter_dev; /* optional device counter added to `counter` (keeps a captured
                                  HIP graph drawing fresh noise on every replay) */
  double gamma;               /* discount for ASVRL_F_RET (trainer.py:161); 0 disables */
  const uint8_t* env_mask;    /* optional [n_envs]: only envs with mask != 0 are processed */
} AsvStepCtl;

/* Outputs of asvrl_env_step (device). Optional members may be NULL. */
typedef struct AsvStepOut {
  float* obs;        /* [n_envs*max_robots][ASVRL_OBS_DIM] packed f32 observation */
  double* obs64;     /* optional [n_envs*max_robots][32] f64 self(7)+objects(25) (compat path) */
  int8_t* obj_cnt;   /* [n_envs*max_robots] objects kept (0..5); -1 = (None, None) */
  double* reward;    /* [n_envs*max_robots] (env.py:242-328) */
  uint8_t* done;     /* [n_envs*max_robots] */
  uint8_t* info;     /* [n_envs*max_robots] ASVRL_INFO_* */
  uint8_t* env_done; /* optional [n_envs] trainer episode end (trainer.py:172) */
  double* stats;     /* optional [8] running sums over finished robot-episodes:
                        return, count, reach-goal, collision, timeout, env-episodes */
} AsvStepOut;

/* Reset parameters (env.py:33-54,72-164, curriculum values from the schedule). */
typedef struct AsvResetCfg {
  int32_t num_robots, num_obs, num_cores, _pad0;
  double min_start_goal_dis, width, height, clear_r;
  double obs_r_lo, obs_r_hi;       /* env.py:39 */
  double v_lo, v_hi;               /* env.py:38 core edge speed */
  double v_rel_max, p_rel;         /* env.py:36-37 */
} AsvResetCfg;

/* ---------------------------------------------------------------- env */

/* MarineNavEnv3.step (env.py:240-333) for every env of the batch in one launch: the N
 * Fossen substeps per robot (wamv.py:204-279, current field env.py:458-501), the sector
 * "LiDAR" object list with top-5 selection and collision test (wamv.py:436-529), COLREGs
 * (wamv.py:324-434) and reward/done/info (env.py:271-331).
 * actions: [n_envs*max_robots][2] f64; discrete actions pass the action index in [0].
 * noise (noise_mode 0): [n_envs*max_robots][max_obs + max_robots][5] f64 draws
 *   [n_px, n_py, n_vx, n_vy, vonmises] per candidate slot (slot k < max_obs: obstacle k,
 *   slot max_obs + j: robot j), in the order Perception makes them (wamv.py:27-40). */
int asvrl_env_step(const AsvParams* params, const AsvEnvState* state, const double* actions,
                   const double* noise, const AsvStepCtl* ctl, const AsvStepOut* out,
                   void* stream);

/* Launch shape of the env-step kernel (asvrl_env_step_ex). Zero members mean "choose":
 *   layout 0: automatic (pair-parallel perception when its LDS fits, else the per-robot sweep),
 *          1: pair-parallel (one lane per (robot, candidate) pair; fails if the LDS does not fit),
 *          2: per-robot sweep (one lane per robot, candidates in a serial loop);
 *   block  threads per workgroup of the pair layout (64, 128 or 256; 0: 256 lanes, or one wave from
 *          16384 envs when an env has at most 8 robots);
 *   envs_per_block  envs per workgroup of the pair layout (0: about 40 robots per group, about 120
 *          when an env has more than 8 robots). */
typedef struct AsvEnvLaunch {
  int32_t layout;
  int32_t block;
  int32_t envs_per_block;
  int32_t max_groups;   /* ABI 19: pair layout as launches of at most this many workgroups, one after another
                           (0 = one launch) -- the rollout's share of the chip beside a learner */
} AsvEnvLaunch;

/* asvrl_env_step with an explicit kernel shape (tests of every shipped layout, A/B tools);
 * launch == NULL is asvrl_env_step. Results do not depend on the shape. */
int asvrl_env_step_ex(const AsvParams* params, const AsvEnvState* state, const double* actions,
                      const double* noise, const AsvStepCtl* ctl, const AsvStepOut* out,
                      const AsvEnvLaunch* launch, void* stream);

/* ABI 27: K open-loop env steps in one launch (asvrl_env_rollout). */
typedef struct AsvRollout {
  int32_t n_steps;        /* K >= 1 */
  int32_t hold_done;      /* 1 (needs trainer_deactivate): an env stops after the step that sets its env_done */
  const double* actions;  /* [K][n_envs*max_robots][2] */
  const double* noise;    /* noise_mode 0: [K][n_envs*max_robots][max_obs+max_robots][5] */
  /* per-step records, every member optional (NULL: not kept) */
  double*  reward;        /* [K][NT], NT = n_envs*max_robots */
  uint8_t* done;          /* [K][NT] */
  uint8_t* info;          /* [K][NT] */
  uint8_t* env_done;      /* [K][n_envs] (trainer_deactivate) */
  float*   obs;           /* [K][NT][ASVRL_OBS_DIM] */
  int8_t*  obj_cnt;       /* [K][NT] */
  double*  rs;            /* [K][ASVRL_NUM_FIELDS][NT] state after each step (placed robots only) */
  int32_t* steps_run;     /* [n_envs] steps this env took (K unless held or masked: 0) */
} AsvRollout;

/* n_steps calls of asvrl_env_step_ex in one launch: step t takes row t of ro->actions (and of ro->noise in
 * noise_mode 0) and draws Philox noise at ctl->counter + t (+ *ctl->counter_dev) -- the values, bit for bit, that
 * n_steps single calls with counter + t compute (replaying a recorded trace, teacher-forced evaluation, action
 * repeat, scoring candidate action sequences). An env group lives inside one workgroup of the pair layout, so
 * the workgroup loops over the steps with the robot state, goals, flags and returns resident in registers and
 * LDS and the buoys staged once; the state returns to HBM after the env's last step. `last` receives the last
 * step's outputs as a single step writes them (with hold_done: each env's end step); stats accumulate as over
 * the single calls. ctl->do_dynamics must be 1; ctl->env_mask is honoured. Record rows of steps an env did not
 * take (masked, or after a hold) are not written: pre-fill them. hold_done is the chain of single steps whose
 * env_mask drops an env after its env_done. launch->max_groups splits the rollout into launches over groups.
 * The sweep layout (robot_params, layout 2, pair LDS too large) runs n_steps single launches instead, each
 * followed by a small record launch (hold_done: with a stream-ordered scratch mask of n_envs bytes). */
int asvrl_env_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                      const AsvStepOut* last, const AsvRollout* ro, const AsvEnvLaunch* launch /* NULL: automatic */,
                      void* stream);

/* MarineNavEnv3.reset (env.py:72-164) for envs with env_mask != 0, sampled on the device
 * with Philox (same rejection rules and iteration caps; not the reference's RandomState
 * stream -- the parity path resets on the host). Follow with asvrl_env_step(do_dynamics=0,
 * env_mask) to produce the reset observation. */
int asvrl_env_reset(const AsvParams* params, const AsvEnvState* state, const AsvResetCfg* cfg,
                    const uint8_t* env_mask, uint64_t seed, uint64_t counter,
                    const uint64_t* counter_dev, void* stream);

/* The training loop's auto-reset in ONE launch: for every env with env_mask[e] != 0, asvrl_env_reset's
 * sampler (one wave) followed by that env's reset observation, computed by the step kernel's phases with
 * ctl (do_dynamics = 0, env_mask = the same mask, Philox noise: noise_mode 1 or 2) into out -- the
 * same values as asvrl_env_reset + the masked asvrl_env_step, without the second launch over all envs.
 * Replaces, for the batched trainer, the reset() + get_observations() pair of MarineNavEnv3.reset
 * (env.py:72-164) that trainer.py calls at an episode end. Requires robot_params == NULL. */
int asvrl_env_reset_observe(const AsvParams* params, const AsvEnvState* state, const AsvResetCfg* cfg,
                            const uint8_t* env_mask, uint64_t seed, uint64_t counter,
                            const uint64_t* counter_dev, const AsvStepCtl* ctl, const AsvStepOut* out,
                            void* stream);

/* Ocean current of env.py:458-501 at n query points xy [n][2] for one env's cores
 * [n_cores][4] -> out [n][3]. Used for the initial velocity of reset_with_eval_config
 * (env.py:609-610); the step kernel evaluates the same field per substep. */
int asvrl_current_field(const double* cores, int32_t n_cores, double core_r, const double* xy,
                        int32_t n, double* out, void* stream);

/* ---------------------------------------------------------------- learner */

/* Quantile-Huber loss of agent.py:406-412 (+ calculate_huber_loss agent.py:701-707) and its
 * gradient w.r.t. the expected quantiles:
 *   delta[b,i,j] = qt[b,j] - qe[b,i]
 *   row_loss[b]  = (1/Np) sum_j sum_i |tau[b,i] - 1{delta<0}| * H_kappa(delta) / kappa
 *   loss[0]      = mean_b row_loss[b]
 *   dqe[b,i]     = grad_scale * d loss / d qe[b,i]
 * qt [B][Np], qe [B][N], tau [B][N] f32. loss may be NULL. */
int asvrl_quantile_huber(const float* qt, const float* qe, const float* tau, int32_t B, int32_t N,
                         int32_t Np, float kappa, float grad_scale, float* row_loss, float* loss,
                         float* dqe, void* stream);

/* C51 categorical projection of agent.py:616-631 (Tz, clamp, b, l/u with the l == u fix,
 * index_add_ of p(u - b) then p(b - l)), bit-identical to the reference's CPU f32 result.
 * pns_a [B][atoms], returns [B], nonterminal [B], support [atoms] -> m [B][atoms]. */
int asvrl_c51_project(const float* pns_a, const float* returns, const float* nonterminal,
                      const float* support, int32_t B, int32_t atoms, float vmin, float vmax,
                      float delta_z, float gamma_n, float* m, void* stream);
/* The same with returns[b * ld_ret] and nonterminal[b * ld_nt] (ABI 21): the columns of the replay rows
 * read in place (the Rainbow update's R^n and nonterminal columns, no copies). */
int asvrl_c51_project_ex(const float* pns_a, const float* returns, int64_t ld_ret, const float* nonterminal,
                         int64_t ld_nt, const float* support, int32_t B, int32_t atoms, float vmin, float vmax,
                         float delta_z, float gamma_n, float* m, void* stream);

/* ---------------------------------------------------------------- fused IQN critic (MFMA) */

/* Critic trunk weights of AC_IQN_model.py:392-408 (concat 256, hidden 128, 64 cosines), the
 * matrices pre-packed into bf16 MFMA A-operand fragments (64 lanes x 8 bf16 per
 * 32x32x16 fragment, in the k order the kernel's register chaining needs -- built by
 * critic_pack.py from the f32 nn.Linear weights). Biases / output row stay f32. */
typedef struct AsvCriticWeights {
  const void* wc_frag;   /* cos_embedding.weight  (256 x 64)  : 32 fragments */
  const void* w1_frag;   /* hidden_layer.weight   (128 x 256) : 64 fragments */
  const void* w2_frag;   /* hidden_layer_2.weight (128 x 128) : 32 fragments */
  const void* w2t_frag;  /* its transpose, for the backward   : 32 fragments */
  const void* w1t_frag;  /* hidden_layer.weight^T (256 x 128) : 64 fragments */
  const float* bc;       /* cos_embedding.bias [256] */
  const float* b1;       /* hidden_layer.bias [128] */
  const float* b2;       /* hidden_layer_2.bias [128] */
  const float* wo;       /* output_layer.weight [128] */
  const float* bo;       /* output_layer.bias [1] */
  /* f32 encoder parameters, read when an IO struct passes observation rows (obs != NULL): the
   * trunk kernels then compute F = observation_processor(obs) (AC_IQN_model.py:284-308,
   * IQN_model.py:80-96) and G = action_encoder(act) (AC_IQN_model.py:468-470) per sample in their
   * prologue instead of reading F / G. NULL when unused. */
  const float* self_w;   /* self_encoder.0.weight (56 x 7), .bias [56] */
  const float* self_b;
  const float* obj_w;    /* object_encoder.0.weight (40 x 5), .bias [40] */
  const float* obj_b;
  const float* ae_w;     /* action_encoder.0.weight (128 x 2), .bias [128] (AC-IQN critic only) */
  const float* ae_b;
} AsvCriticWeights;

/* bf16 row-major activations the TRAIN mode writes for the weight gradients
 * (dW = dZ^T X per layer), R = B*N rows. */
typedef struct AsvCriticActs {
  void* cos;   /* [R][64]   cos(tau pi k)            -> d cos_embedding.weight with dzc */
  void* h0;    /* [R][256]  F * c                    -> d hidden_layer.weight with dz1 */
  void* dzc;   /* [R][256]  dL/d(cos_embedding pre-activation) */
  void* h1g;   /* [R][128]  h1 * G                   -> d hidden_layer_2.weight with dz2 */
  void* dz1;   /* [R][128]  dL/d(hidden_layer pre-activation) */
  void* h2;    /* [R][128]  relu(hidden_layer_2)     -> d output_layer.weight with dq */
  void* dz2;   /* [R][128]  dL/d(hidden_layer_2 pre-activation) */
  float* dq;   /* [R]       dL/dq */
  float* wout_part; /* optional, AC-IQN TRAIN: [asvrl_critic_wout_groups(B, N)][129] per-workgroup
                       partials of output_layer's dW (128) | db, reduced in the kernel from f32 h2 and
                       dq (h2 and dq may then be NULL; reduce them with asvrl_partial_sums, nw 128, nb 1) */
} AsvCriticActs;

/* Number of [129] output-layer gradient partials asvrl_critic_train writes to acts->wout_part. */
int32_t asvrl_critic_wout_groups(int32_t B, int32_t N);

/* Fill the five bf16 fragment images of w (wc_frag .. w1t_frag) from the row-major f32
 * weights cos_embedding.weight (256 x 64), hidden_layer.weight (128 x 256) and
 * hidden_layer_2.weight (128 x 128) (AC_IQN_model.py:398-402). One launch. */
int asvrl_critic_pack(const float* wc, const float* w1, const float* w2, const AsvCriticWeights* w, void* stream);

/* Inputs / outputs of one critic launch. F (B x 256) = observation_processor features,
 * G (B x 128) = action_encoder features, taus (B x N); N in {8, 16, 32}. */
typedef struct AsvCriticIO {
  const float* F;          /* [B][256], or NULL with obs set */
  const float* G;          /* [B][128], or NULL with act set */
  const float* obs;        /* optional packed observation rows (ASVRL_OBS_DIM layout) at obs[b*ld_obs] */
  int64_t ld_obs;
  const float* act;        /* optional actions (2 f32) at act[b*ld_act] */
  int64_t ld_act;
  void* xb;                /* TRAIN optional: bf16 [B][32] copy of obs columns 0..31 (encoder wgrad operand) */
  const float* taus;
  int32_t B, N, Np;
  float kappa;
  const float* q_targets;  /* TRAIN: [B][Np], or NULL with q_next set: */
  const float* q_next;     /*   q_targets = rewards + gamma * q_next * (1 - dones) (agent.py:399-400) */
  const float* rewards;    /*   B values at stride ld_rd floats */
  const float* dones;
  int64_t ld_rd;
  float gamma;
  float dq;                /* ACTOR: dL/dq of every row (-1/(B*N) for actor_loss = -mean q) */
  float* q;                /* [B*N] (FWD: required) */
  float* row_loss;         /* TRAIN: [B*N], sums to B*Np*loss */
  float* dF;               /* TRAIN optional: dL/dF [B][256] */
  float* dG;               /* TRAIN / ACTOR optional: dL/dG [B][128] */
  void* dzF;               /* TRAIN optional: bf16 [B][256] dF * 1[F > 0] (encoder pre-activation grad) */
  float* dzG;              /* TRAIN optional: [B][128] dG * 1[G > 0] (action-encoder pre-activation grad) */
  const float* w_ae;       /* ACTOR with dA: action_encoder.weight [128][2] */
  float* dA;               /* ACTOR optional: dL/d(action) [B][2] = W_ae^T (dG * 1[G > 0]) */
  float* tile_loss;        /* optional [B*N/32]: per 32-row tile, TRAIN writes sum(row_loss) * loss_scale
                              (the critic loss with loss_scale = 1/(B*Np)), ACTOR sum(q) * loss_scale
                              (the actor loss with -1/(B*N)); sum them with asvrl_partial_sums
                              (a segment with nw = 1, groups = tiles) */
  float loss_scale;
} AsvCriticIO;

/* Critic.forward (AC_IQN_model.py:462-480): q [B*N]. */
int asvrl_critic_forward(const AsvCriticWeights* w, const AsvCriticIO* io, void* stream);

/* Critic update of train_AC_IQN (agent.py:395-414): forward, the quantile-Huber loss against
 * the targets and its backward in one launch; acts receive the activations for the weight
 * gradients. */
int asvrl_critic_train(const AsvCriticWeights* w, const AsvCriticIO* io, const AsvCriticActs* acts,
                       void* stream);

/* Per-workgroup weight-gradient partials of asvrl_critic_train_fused, [groups][M*K + M] per layer
 * (dW row-major in the layer's own feature order, then db); groups = asvrl_critic_fused_groups.
 * Sum them over the groups with asvrl_partial_sums (nw = M*K, nb = M, stride = M*K + M). */
typedef struct AsvCriticParts {
  float* cos_emb;   /* cos_embedding   (256 x 64): [groups][16384 + 256] */
  float* hidden;    /* hidden_layer    (128 x 256): [groups][32768 + 128] */
  float* hidden2;   /* hidden_layer_2  (128 x 128): [groups][16384 + 128] */
  float* out;       /* output_layer    (1 x 128):  [groups][128 + 1] */
  /* optional (ABI 16; asvrl_critic_train_fused only, NULL = not formed, then dzF / dzG / xb as
   * before): the encoders' gradients from the kernel's own per-sample dzF / dzG, without them
   * leaving the chip.
   * enc:  observation encoders, folded over the five objects (the contiguous layout of
   *       AC_IQN_model.py's self_encoder / object_encoder parameters):
   *       [groups][self_w 56x7 | self_b 56 | obj_w 40x5 | obj_b 40] = [groups][688]
   * aenc: action encoder (2 -> 128): [groups][w 128x2 | b 128] = [groups][384] */
  float* enc;
  float* aenc;
} AsvCriticParts;

/* Workgroups (= partial groups) of asvrl_critic_train_fused for B samples x N quantiles: one per
 * CU at most, each taking rounds of 64 rows (32 in the f32 build). */
int32_t asvrl_critic_fused_groups(int32_t B, int32_t N);

/* The critic update of train_AC_IQN (agent.py:395-414) WITH its trunk weight gradients, in one
 * persistent launch: encoders from io->obs / io->act, forward, quantile-Huber loss against
 * r + gamma q_next (1 - d) (io->q_next [B][N], rewards / dones at stride ld_rd), backward, and
 * per-workgroup dW / db partials of the four trunk layers (parts); per-sample dzF / dzG and xb for
 * the encoder gradients, per-tile loss partials (tile_loss) as asvrl_critic_train. N' must equal N;
 * B*N a multiple of the round size. No activation goes to HBM. */
int asvrl_critic_train_fused(const AsvCriticWeights* w, const AsvCriticIO* io, const AsvCriticParts* parts,
                             void* stream);

/* asvrl_critic_train_fused with the target critic's forward in the same launch (ABI 20; replaces the
 * separate asvrl_critic_forward(target) of train_AC_IQN, agent.py:396-400): each workgroup first computes
 * q_next = Critic_target(tio->obs, tio->act, tio->taus) (AC_IQN_model.py:462-480) for exactly the samples
 * its rounds update into io->q_next, then runs the update reading them. tw: the target critic (with its
 * encoders); tio: B and N as io. With kernel variant 4 (asvrl_critic_fused_variant; the default) the target
 * pass is asvrl_critic_forward's own tile: q_next bit for bit what asvrl_critic_forward(tw, tio) gives; with
 * variant 8 it is the update kernel's own forward phases: the same rounding points, f32 sums in another
 * order. */
int asvrl_critic_train_fused_tq(const AsvCriticWeights* w, const AsvCriticIO* io, const AsvCriticParts* parts,
                                const AsvCriticWeights* tw, const AsvCriticIO* tio, void* stream);

/* ABI 23: the kernel asvrl_critic_train_fused(_tq) launch where both forms take the shape (bf16 build, N = 32,
 * parts->enc and parts->aenc set, no dzF / dzG / xb): 8 = two waves per SIMD (512-thread workgroups), 4 = one
 * wave per SIMD (the round-5 kernel; the default: variant 8 measured 11 % slower). Results
 * agree within f32 summation order, not bit for bit.
 * v < 0 only queries; returns the previous setting, or -1 (asvrl_last_error) for any other v. Process-wide. */
int32_t asvrl_critic_fused_variant(int32_t v);

/* Actor update's critic pass (agent.py:419-425): forward, then the backward of
 * sum_rows dq * q to G (dG) and through the action encoder to the action (dA). */
int asvrl_critic_actor_grad(const AsvCriticWeights* w, const AsvCriticIO* io, void* stream);

/* ---------------------------------------------------------------- IQN (IQN_model.py, agent.py:227-256, 434-476) */

/* IQN_Policy has the critic's trunk without the action encoder (h1 feeds hidden_layer_2
 * directly, IQN_model.py:106-108) and an output_layer 128 -> A (A <= 32 actions). Its trunk
 * uses AsvCriticWeights (wo / bo unused); the head is described here. */
#define ASVRL_IQN_MAX_ACTIONS 32
typedef struct AsvIqnHead {
  const void* wo_frag;  /* output_layer.weight padded to 32 x 128, chained fragment order: 8 fragments */
  const float* wo;      /* output_layer.weight [A][128] f32 (the TRAIN backward) */
  const float* bo;      /* output_layer.bias [A] */
  int32_t n_actions;    /* A */
} AsvIqnHead;

/* Pack the trunk images (as asvrl_critic_pack) and the head image in one launch. */
int asvrl_iqn_pack(const float* wc, const float* w1, const float* w2, const float* wout,
                   const AsvCriticWeights* w, const AsvIqnHead* head, void* stream);

/* Inputs / outputs of one IQN launch. Rows are (sample b, tau n), R = B*N. */
typedef struct AsvIqnIO {
  const float* F;          /* [B][256] observation features, or NULL with obs set */
  const float* obs;        /* optional packed observation rows at obs[b*ld_obs] (encoders in-kernel) */
  int64_t ld_obs;
  void* xb;                /* TRAIN optional: bf16 [B][32] copy of obs columns 0..31 */
  const float* taus;       /* [B*N]; ACT: may be NULL = drawn in the kernel (Philox, uniform [0,1)) */
  int32_t B, N, Np;        /* N in {8,16,32} (ACT: N = K = 32); Np = target quantiles per sample (TRAIN) */
  float kappa;             /* Huber threshold (1.0, agent.py:458) */
  const float* q_next;     /* TRAIN: [B][Np] max over actions of the target quantiles (asvrl_iqn_forward_max) */
  const float* actions;    /* TRAIN: action index of sample b at actions[b*ld_rd] (f32, replay row column) */
  const float* rewards;    /* TRAIN: rewards[b*ld_rd] */
  const float* dones;      /* TRAIN: dones[b*ld_rd] */
  int64_t ld_rd;
  float gamma;
  float* q;                /* FORWARD_MAX: [R] max_a Q(row, a); TRAIN optional: [R] Q(row, a_b) */
  float* row_loss;         /* TRAIN optional: [R] sum over target quantiles of the quantile-Huber term */
  void* dzF;               /* TRAIN: bf16 [B][256] dL/dF * 1[F > 0] (encoder pre-activation grad) */
  void* dz_out;            /* TRAIN: bf16 [R][32] dL/d(output pre-activation): dq at the taken action, else 0 */
  float* tile_loss;        /* TRAIN optional: [R/32] per-tile sum(row_loss) * loss_scale */
  float loss_scale;
  /* ACT (act_iqn, agent.py:227-256): action = argmax_a mean_n Q(b, n, a), epsilon-greedy */
  double* act_out;         /* [B] action index as f64 at act_out[b*ld_act] */
  int64_t ld_act;
  const int64_t* step_dev; /* device step counter for the epsilon schedule and the RNG counter */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;
  uint64_t seed;
} AsvIqnIO;

/* Target pass of train_IQN (agent.py:451-452): q[row] = max_a Q(row, a). */
int asvrl_iqn_forward_max(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io, void* stream);

/* Local pass of train_IQN (agent.py:455-468): forward, gather at the taken action, the
 * quantile-Huber loss against r + gamma * q_next * (1 - d), and the whole trunk backward
 * (two launches). acts: h1g holds h1; dq is optional. */
int asvrl_iqn_train(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io,
                    const AsvCriticActs* acts, void* stream);

/* train_IQN's local pass (agent.py:455-468) WITH the trunk and output-layer weight gradients, in
 * one persistent launch (asvrl_critic_train_fused's kernel on IQN_Policy's trunk): encoders from
 * io->obs, forward, gather at io->actions, quantile-Huber loss, backward, per-workgroup partials
 * (parts; parts->out is [groups][32*128 + 32], output rows >= A zero), dzF / xb / tile_loss.
 * dz_out is not written; N' must equal N; groups = asvrl_critic_fused_groups(B, N). */
int asvrl_iqn_train_fused(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io,
                          const AsvCriticParts* parts, void* stream);
/* ABI 24: the same launch with train_IQN's target (agent.py:451-452: qnetwork_target(next_states, taus').max over
 * the actions) computed inside it first: each workgroup forms q_next for exactly the samples it updates (the
 * IQN_MAX tile of asvrl_iqn_forward_max, bit-identical) into io->q_next, then the update reads it. tw / thead:
 * the target network's images and head; tio: taus (the target's tau'), obs (next-observation rows), B and N as
 * io. Replaces asvrl_iqn_forward_max + asvrl_iqn_train_fused. */
int asvrl_iqn_train_fused_tq(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io,
                             const AsvCriticParts* parts, const AsvCriticWeights* tw, const AsvIqnHead* thead,
                             const AsvIqnIO* tio, void* stream);

/* act_iqn (agent.py:227-256) for every row of F with K = 32 quantile samples per state. */
int asvrl_iqn_act(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io, void* stream);

/* The window form of asvrl_iqn_act (new entry points only: the ABI version stays 29). What it adds to the pass: */
typedef struct AsvIqnActEx {
  float cvar;              /* in (0, 1]: every tau of the pass, drawn or given, is multiplied by it before the cosine
                              embedding (calc_cos's taus * cvar, IQN_model.py:68); 1: asvrl_iqn_act's bits */
  int32_t robots_per_env;  /* >= 1: row b belongs to env b / robots_per_env (env_mask) */
  int64_t step_add;        /* the tau draw, the epsilon schedule and the exploration draw use *step_dev + step_add */
  double* act_pair;        /* optional [B][2]: (action index, 0.0), what asvrl_env_step_ex takes with
                              is_continuous = 0 */
  double* rec_row;         /* optional [B][2]: the same pair, written only for rows of envs with env_mask != 0 */
  const uint8_t* env_mask; /* optional [B / robots_per_env]; NULL: every env */
  float* qmean_out;        /* optional [B][ld_q]: column a < n_actions = mean over the 32 taus of Q(s, tau, a), act_iqn's
                              quantiles.mean(dim=1); columns >= n_actions are not written */
  int64_t ld_q;
} AsvIqnActEx;
/* io as asvrl_iqn_act's, except that io->act_out may be NULL when ex->act_pair or ex->rec_row is given. */
int asvrl_iqn_act_ex(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io, const AsvIqnActEx* ex,
                     void* stream);
/* sizeof(AsvIqnActEx) as compiled. */
int64_t asvrl_iqn_act_ex_struct_size(void);

/* A risk level per row instead of AsvIqnActEx's one scalar (new entry points only: the ABI version stays 29). Row b's 32
 * quantile fractions, drawn or given, are multiplied by level[b] before the cosine embedding. */
#define ASVRL_IQN_RISK_ROWS 1      /* level[b] = cvar_rows[b] */
#define ASVRL_IQN_RISK_ADAPTIVE 2  /* level[b] from io->obs row b (self 7 | objects 5 x 5 (px, py, vx, vy, r), nearest
                                      first | mask 5), in f32: 1 if mask[0] < 0.5 (no object); otherwise
                                      d = sqrt(px0^2 + py0^2) - r0 - margin, and 1 if d >= near, else max(d / near, floor)
                                      (the rule agent.py:342-358 keeps commented out, with a floor) */
typedef struct AsvIqnRisk {
  int32_t mode;            /* ASVRL_IQN_RISK_ROWS or ASVRL_IQN_RISK_ADAPTIVE */
  float near;              /* adaptive: > 0 (the reference's 10) */
  float margin;            /* adaptive: finite (the reference's 2.8) */
  float floor;             /* adaptive: in (0, 1]; the reference's rule has none */
  const float* cvar_rows;  /* rows: [B], each in (0, 1] (not checked: device memory) */
  float* cvar_out;         /* optional [B]: the level every row used */
} AsvIqnRisk;
/* asvrl_iqn_act_ex with the factor taken from risk: ex->cvar must be 1. ex->act_pair still receives (index, 0.0), the
 * pair the env step takes; ex->rec_row receives (index, level used), the f32 level widened exactly. The adaptive
 * mode needs io->obs (precomputed features carry no observation row). */
int asvrl_iqn_act_risk(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io, const AsvIqnActEx* ex,
                       const AsvIqnRisk* risk, void* stream);
/* sizeof(AsvIqnRisk) as compiled. */
int64_t asvrl_iqn_risk_struct_size(void);

/* The quantile samples behind act_iqn's decisions (act_iqn's (action, quantiles, taus), agent.py:227-256), read out
 * after the fact (new entry points only: the ABI version stays 29). The pass is asvrl_iqn_act_ex's tile -- the same
 * workgroup, the same MFMA order -- so the action values it recomputes are the bits the act launch chose from; it
 * draws no exploration and writes no action. io: obs (or F), ld_obs, B = M rows, N = 32, taus ([M][32] or NULL =
 * drawn) and seed; io->step_dev is not read. The rows are laid out [steps][rows_per_step]: row m is robot slot
 * n = m % rows_per_step at step t = step0 + m / rows_per_step, and a drawn fraction is act_tau's Philox draw on
 * (n * 32 + sample, t, seed): what the window's act launch over rows_per_step rows drew at step t. */
typedef struct AsvIqnDist {
  int32_t rows_per_step;   /* >= 1 */
  float cvar;              /* in (0, 1]: every fraction times cvar; must be 1 with level_rows */
  int64_t step0;
  const float* level_rows; /* optional [M], each in (0, 1] (device memory: not checked): row m's fractions times it.
                              A value outside the range only scales that row's fractions -- no address depends on it;
                              the device evaluation relies on that for the rows of slots that did not act */
  const double* actions;   /* optional [M][2]: the selected action is column 0 (the windows' actions record); NULL:
                              the recomputed arg-max. An index outside 0..A-1 gives a NaN z_out row */
  float* z_out;            /* optional [M][32]: the selected action's quantile values in sample order */
  float* tau_out;          /* optional [M][32]: the fractions used, after the level */
  float* all_out;          /* optional [M][32][ld_a]: every action's values, columns >= n_actions not written */
  int64_t ld_a;            /* >= n_actions with all_out */
  int32_t* greedy_out;     /* optional [M]: the first arg-max of the 32-sample sums, whatever actions says */
  float* qmean_out;        /* optional [M][ld_q]: the action values, as AsvIqnActEx.qmean_out */
  int64_t ld_q;            /* >= n_actions with qmean_out */
} AsvIqnDist;
int asvrl_iqn_dist(const AsvCriticWeights* w, const AsvIqnHead* head, const AsvIqnIO* io, const AsvIqnDist* dist,
                   void* stream);
/* sizeof(AsvIqnDist) as compiled. */
int64_t asvrl_iqn_dist_struct_size(void);

/* What stands in front of asvrl_critic_forward (N = 32, obs and act) when the AC-IQN critic's quantiles are read
 * out at recorded actions: the fractions and the f32 copy of the f64 action pairs, in one launch. Row m is robot
 * slot n = m % rows_per_step at step t = step0 + m / rows_per_step; taus_out[m][j] is the Philox draw on
 * (n * 32 + j, t, seed) of a stream of its own (not act_tau's), uniform [0, 1). */
typedef struct AsvDistPrepare {
  int32_t rows;            /* M >= 0 */
  int32_t rows_per_step;   /* >= 1 */
  int64_t step0;
  uint64_t seed;
  float* taus_out;         /* optional [M][32] */
  const double* actions;   /* optional [M][2] f64, with act_out */
  float* act_out;          /* optional [M][2]: (float) of the pair; exact for an actor's f32 output widened */
} AsvDistPrepare;
int asvrl_dist_prepare(const AsvDistPrepare* p, void* stream);
/* sizeof(AsvDistPrepare) as compiled. */
int64_t asvrl_dist_prepare_struct_size(void);

/* ---------------------------------------------------------------- replay (replay_buffer.py) */

/* ReplayBuffer.add (replay_buffer.py:22-24) for every robot that acted in the last step
 * (obj_cnt_next >= 0), in slot order, into a ring of `capacity` rows of ASVRL_TR_DIM f32.
 * ring_state: int64[2] = {head, size} in device memory (updated by the call, so the call
 * is capturable in a HIP graph). work: int32[ceil(n / 256) + 1] scratch, ZERO before the first call
 * (work[0] is the launch's arrival counter, work[1] the blocks' running row count; the call leaves both zero
 * again). One launch. */
int asvrl_replay_push(const float* obs_prev, const float* obs_next, const int8_t* obj_cnt_next,
                      const double* actions, int32_t action_dim, const double* reward,
                      const uint8_t* done, int32_t n, float* ring, int64_t capacity,
                      int64_t* ring_state, int32_t* work, void* stream);
/* asvrl_replay_push with actions rows action_ld doubles apart (the first action_dim used) that also
 * writes the new {head, size} to `snap` (int64[2], optional: the ring snapshot a concurrent learner
 * samples against) and increments *counter_inc (optional: the env step counter), in the same launch
 * (ABI 18). */
int asvrl_replay_push_ex(const float* obs_prev, const float* obs_next, const int8_t* obj_cnt_next,
                         const double* actions, int32_t action_dim, int64_t action_ld, const double* reward,
                         const uint8_t* done, int32_t n, float* ring, int64_t capacity,
                         int64_t* ring_state, int32_t* work, int64_t* snap, int64_t* counter_inc,
                         void* stream);

/* ReplayBuffer.sample (replay_buffer.py:26-45): gather B rows. With `indices` (host-chosen,
 * deque order: 0 = oldest) the rows are exactly those; with indices == NULL, B positions are
 * drawn uniformly (with replacement) by Philox(seed, counter + *counter_dev), skipping the
 * oldest entries that a push of up to `guard` rows running concurrently could overwrite
 * (guard = 0: none). ring_state may be a snapshot {head, size} taken before that push.
 * out [B][ASVRL_TR_DIM]; out_slots optional [B]. taus (optional): tau_sets x [B][tau_n] quantile
 * fractions U[0, 1) for the update (the torch.rand of AC_IQN_model.py:419 / IQN_model.py:62), drawn
 * from Philox(seed, counter + *counter_dev) in the same launch. */
int asvrl_replay_sample(const float* ring, int64_t capacity, const int64_t* ring_state,
                        const int64_t* indices, int32_t B, uint64_t seed, uint64_t counter,
                        const uint64_t* counter_dev, int64_t guard, float* out, int64_t* out_slots,
                        float* taus, int32_t tau_sets, int32_t tau_n, void* stream);

/* Host-side index copy helper for a ring with known (host) head/size: write rows given by
 * slot into the ring (used by the compat ReplayBuffer.add, one transition per call). */
int asvrl_replay_write_rows(const float* rows, const int64_t* slots, int32_t n, float* ring,
                            void* stream);

/* ---------------------------------------------------------------- prioritised n-step replay
 * Rainbow's ReplayMemory + SegmentTree (policy/replay_memory_rainbow.py:14-196) in HBM. All members
 * are device pointers the caller allocates (zero-initialised, maxp[0] = 1.0f); the struct itself is
 * read on the host at each call. */
typedef struct AsvPer {
  float* rows;          /* [capacity][ASVRL_PER_DIM] */
  float* tree;          /* [2 * tree_leaves - 1] sum tree, leaves at tree_leaves - 1 (:17) */
  int64_t* state;       /* [4] {index, full, reserved, anomaly count (rejections left after 64 redraws,
                           unsorted priority updates)} */
  int32_t* t;           /* [stride] per-stream timestep counter (ReplayMemory.t, :107,139) */
  float* maxp;          /* [1] SegmentTree.max (:22) */
  uint8_t* dirty;       /* [max(1, tree_leaves / 2048)] dirty 2048-leaf blocks (cleared by the rebuild) */
  int64_t capacity;     /* slots, a multiple of stride */
  int64_t tree_leaves;  /* next power of two >= capacity, <= 2^22 */
  int32_t stride;       /* slots per time step: 1 = the reference's single sequence; E*R = one stream per robot */
  int32_t n_step;       /* n (3, :105) */
  double discount;      /* 0.99 (:104) */
  float priority_weight;    /* beta 0.4 (:106) */
  float priority_exponent;  /* omega 0.5 (:107) */
  int32_t deferred;     /* 0: the reference's tree (every append at max priority, rejection sampling);
                           1: a slot's priority enters the tree when its n-step window is complete */
  int32_t _pad0;
} AsvPer;

/* ReplayMemory.append (:132-139) for n = m * stride rows (m time steps, rows time-major): robot
 * k % stride appends obs[k] (packed ASVRL_OBS_DIM row), action actions[k*action_dim], reward[k],
 * terminal done[k] at max priority when obj_cnt[k] >= 0, else a blank slot of priority 0 (deferred: the
 * priority is kept in the slot and set on the leaf n steps later, when the window is complete); then
 * the dirty subtrees are rebuilt and the ring advances by n. Three launches. */
int asvrl_per_push(const AsvPer* per, const float* obs, const int8_t* obj_cnt, const double* actions,
                   int32_t action_dim, const double* reward, const uint8_t* done, int32_t n, void* stream);
/* ABI 25: the same, and the device env-step counter step_counter[0] (int64) advanced by one in its last launch
 * (the batched loop's step count, trainer.py:172; NULL: not advanced) */
int asvrl_per_push_ex(const AsvPer* per, const float* obs, const int8_t* obj_cnt, const double* actions,
                      int32_t action_dim, const double* reward, const uint8_t* done, int32_t n, int64_t* step_counter,
                      void* stream);
/* The push of a whole rollout window (new entry point only: the ABI version stays 29): asvrl_per_push_ex on
 * n = K * stride rows (K time steps, time-major: one thread walks each robot's stream in order, so the ring, the
 * tree and the per-stream timesteps are those of K single pushes), with step_counter[0] advanced by counter_by
 * (>= 1; K for a window) in the last launch instead of by one. step_counter may be NULL. */
int asvrl_per_push_window(const AsvPer* per, const float* obs, const int8_t* obj_cnt, const double* actions,
                          int32_t action_dim, const double* reward, const uint8_t* done, int32_t n,
                          int64_t* step_counter, int64_t counter_by, void* stream);

/* ReplayMemory.sample (:157-192): B stratified draws (segment b: uniform in [b*seg, (b+1)*seg) with
 * seg = total / B in f32, the value in f64), SegmentTree.find, the validity rule of :163 (window
 * behind the write head, not the head slot, prob != 0), the n-step window with blanking at later
 * episode starts. uniforms (device f64 [B], optional): the reference's U(0,1) draws, one attempt;
 * otherwise Philox(seed, counter + *counter_dev) with up to 64 per-segment redraws.
 * out [B][ASVRL_TR_DIM]: obs 40 | n-th next obs 40 | action, 0 | R^n | nonterminal |
 * w = (cap * p)^-beta (before the batch-max normalisation) | p = prob / total | data index | 0.
 * out_tree_idx [B] int64: tree indices for asvrl_per_update. One launch. */
int asvrl_per_sample(const AsvPer* per, int32_t B, const double* uniforms, uint64_t seed, uint64_t counter,
                     const uint64_t* counter_dev, float* out, int64_t* out_tree_idx, void* stream);
/* ABI 25: the same, and each draw's weight also into weights[B] (contiguous, for asvrl_per_normalise). */
int asvrl_per_sample_ex(const AsvPer* per, int32_t B, const double* uniforms, uint64_t seed, uint64_t counter,
                        const uint64_t* counter_dev, float* out, int64_t* out_tree_idx, float* weights, void* stream);
/* ABI 25: weights / weights.max() (:191) into the weight column (84) of asvrl_per_sample_ex's B rows, from its
 * contiguous weights, in one launch (the quotients of the reference's expression bit for bit). */
int asvrl_per_normalise(float* rows, const float* weights, int32_t B, void* stream);

/* ReplayMemory.update_priorities (:194-196): leaf tree_idx[i] = values[i] ** priority_exponent
 * (raw != 0: values already exponentiated), duplicates resolved last-wins (tree_idx as sampled, in
 * non-decreasing order), SegmentTree.max updated, dirty subtrees rebuilt. Three launches. */
int asvrl_per_update(const AsvPer* per, const int64_t* tree_idx, const float* values, int32_t B, int32_t raw,
                     void* stream);
/* ABI 25: the same, and in its last launch values_mean[0] = the mean of values (a fixed summation order; the
 * train step's reported loss, agent.py:639) and learn_counter[0] (int64) += 1; either may be NULL. */
int asvrl_per_update_ex(const AsvPer* per, const int64_t* tree_idx, const float* values, int32_t B, int32_t raw,
                        float* values_mean, int64_t* learn_counter, void* stream);

/* ---------------------------------------------------------------- Rainbow (Rainbow_model.py, agent.py)
 * NoisyLinear weights and the dueling C51 head. A network's noisy tensors are described by up to 16
 * segments (weight, bias of each layer); off[k] is the flat offset of segment k (off[n] = total). */
#define ASVRL_MAX_NOISY_SEGS 16
typedef struct AsvNoisySeg {
  const float* mu;      /* weight_mu / bias_mu */
  const float* sigma;   /* weight_sigma / bias_sigma */
  float* eps;           /* weight_epsilon / bias_epsilon (written by asvrl_noisy_reset) */
  float* out;           /* composed mu + sigma * eps */
  const float* dout;    /* backward: gradient of out */
  float* dmu;           /* backward: written with dout */
  float* dsigma;        /* backward: written with dout * eps */
} AsvNoisySeg;

typedef struct AsvNoisySegs {
  int32_t n;
  int32_t _pad0;
  int64_t off[ASVRL_MAX_NOISY_SEGS + 1];
  AsvNoisySeg seg[ASVRL_MAX_NOISY_SEGS];
} AsvNoisySegs;

/* NoisyLinear.forward in training mode (Rainbow_model.py:47-51) for every segment: out = mu + sigma * eps;
 * backward != 0: dmu = dout, dsigma = dout * eps (assigned, the parameters' only use). One launch. */
int asvrl_noisy_compose(const AsvNoisySegs* segs, int32_t backward, void* stream);
/* ABI 26: the backward of asvrl_noisy_compose that also leaves the squared norm of the gradients it writes
 * (dmu^2 + dsigma^2) as asvrl_noisy_backward_norm_parts(segs) f64 per-workgroup partials in sq_parts (a fixed
 * order): with the reduction's own partials (asvrl_partial_sums_norm) the clip norm of asvrl_adam_step. */
int32_t asvrl_noisy_backward_norm_parts(const AsvNoisySegs* segs);
int asvrl_noisy_backward_norm(const AsvNoisySegs* segs, double* sq_parts, void* stream);

/* reset_noise() of every layer (Rainbow_model.py:35-45,141-145) with (weight, bias) segment pairs:
 * f(x) = sign(x) sqrt|x| of N(0, 1) Philox draws (seed, *counter_dev), eps_w = f(eps_out) f(eps_in)^T,
 * eps_b = f(eps_out), and out = mu + sigma * eps in the same launch. in/out_features: HOST int32
 * [n/2] (in <= 256). One workgroup per 16 output units. */
int asvrl_noisy_reset(const AsvNoisySegs* segs, const int32_t* in_features, const int32_t* out_features,
                      uint64_t seed, const int64_t* counter_dev, void* stream);

typedef struct AsvRainbowHeadIO {
  const float* v;           /* [N][ldv] value logits (51) */
  int64_t ldv;
  const float* a;           /* [N][lda] advantage logits (25 x 51, action-major) */
  int64_t lda;
  int32_t N, atoms, actions_n, _pad0;   /* atoms 51, actions_n 25 */
  const float* support;     /* [51] */
  /* act: argmax_a sum softmax(q[a]) z (agent.py:320), epsilon-greedy when step_dev != NULL */
  double* act_out;          /* optional [N] action as f64 at act_out[row * ld_act] */
  int64_t ld_act;
  int64_t* act_idx;         /* optional [N] greedy action (act) / a* input (pick) */
  const int64_t* step_dev;
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;
  uint64_t seed;
  float* p_out;             /* pick: [N][51] softmax(q[a*]) */
  /* loss */
  const float* actions;     /* [N] at actions[row * ld_rd] (replay row column) */
  const float* weights;     /* [N] importance weights at weights[row * ld_rd] */
  int64_t ld_rd;
  const float* m;           /* [N][51] projected target distribution */
  float* loss;              /* [N] per-sample loss */
  float* dv;                /* [N][51] d(grad_scale * sum_b w_b loss_b) / dv */
  float* da;                /* [N][1275] ... / da */
  float grad_scale;         /* 1 / B for the mean */
  int32_t _pad1;
} AsvRainbowHeadIO;

/* Dueling head q = v + a - mean_a(a) (Rainbow_model.py:128-134) per row: softmax over atoms per action,
 * expected value, argmax (first maximum); epsilon-greedy exploration (agent.py:318-322) with the linear
 * schedule of the device step counter when step_dev != NULL. One wave per two rows. */
int asvrl_rainbow_act(const AsvRainbowHeadIO* io, void* stream);
/* p(s', a*) = softmax(q[a*]) (agent.py:611-612), a* = act_idx[row]. One wave per row. */
int asvrl_rainbow_pick(const AsvRainbowHeadIO* io, void* stream);
/* loss_b = -sum m log softmax(q[a_b]) (agent.py:633) and the gradients of grad_scale * sum_b w_b loss_b
 * with respect to v and a. One wave per row. */
int asvrl_rainbow_loss(const AsvRainbowHeadIO* io, void* stream);

/* Rainbow_Policy (Rainbow_model.py:56-139) as one kernel per 32-row tile: encoders, both streams, the
 * dueling combine and the C51 head, bf16 MFMA operands (f32 in libasvrl_f32.so). The weights are
 * fragment images packed from the COMPOSED NoisyLinear weights (asvrl_noisy_compose / _reset, then
 * asvrl_rainbow_pack), including the action-mean of output_layer_a (mean_k a[k] as one more layer). */
typedef struct AsvRainbowSrc {   /* f32 row-major [out][in] */
  const float *self_w, *self_b, *obj_w, *obj_b;            /* self_encoder.0 (56 x 7), object_encoder.0 (40 x 5) */
  const float *w_v1, *b_v1, *w_a1, *b_a1;                  /* hidden_layer_v / _a (128 x 256), composed */
  const float *w_v2, *b_v2, *w_a2, *b_a2;                  /* hidden_layer_v_2 / _a_2 (128 x 128) */
  const float *w_vo, *b_vo, *w_ao, *b_ao;                  /* output_layer_v (51 x 128), output_layer_a (1275 x 128) */
} AsvRainbowSrc;

/* The packed images (operand element type; biases f32). Sizes in elements: enc 8192, v1 / a1 32768,
 * v2 / a2 16384, vo / mo 8192, ao 204800; b_enc 256, b_v1p .. b_a2p 128, b_vop / b_mop 64, b_aop 1600.
 * The backward's transposed images (train only; may be NULL otherwise): vot / mot 8192 (mot holds
 * -mean_k), aot 204800, v2t / a2t 16384, v1t / a1t 32768. */
typedef struct AsvRainbowImgOut {
  void *enc, *v1, *a1, *v2, *a2, *vo, *mo, *ao;
  float *b_enc, *b_v1p, *b_a1p, *b_v2p, *b_a2p, *b_vop, *b_mop, *b_aop;
  void *vot, *mot, *aot, *v2t, *a2t, *v1t, *a1t;
} AsvRainbowImgOut;
typedef struct AsvRainbowImg {   /* the same buffers, read-only */
  const void *enc, *v1, *a1, *v2, *a2, *vo, *mo, *ao;
  const float *b_enc, *b_v1p, *b_a1p, *b_v2p, *b_a2p, *b_vop, *b_mop, *b_aop;
  const void *vot, *mot, *aot, *v2t, *a2t, *v1t, *a1t;
} AsvRainbowImg;

typedef struct AsvRainbowNetIO {
  const float* x;           /* [N] packed observation rows at x[row * ldx] (16-byte aligned, ldx >= 40) */
  int64_t ldx;
  int32_t N, _pad0;
  const float* support;     /* [51] */
  double* act_out;          /* act: [N] action as f64 at act_out[row * ld_act] */
  int64_t ld_act;
  int64_t* act_idx;         /* argmax: [N] greedy action out; pick: a* in; act: optional greedy out */
  const int64_t* step_dev;  /* act: epsilon schedule on the device step counter (NULL: greedy) */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;
  uint64_t seed;
  float* p_out;             /* pick: [N][51] softmax(q[a*]) */
  /* train (agent.py:613-636): loss and backward of mean_b w_b loss_b on the rows x (= s) */
  const float* actions;     /* [N] taken action at actions[row * ld_rd] (replay row column) */
  const float* weights;     /* [N] importance weights at weights[row * ld_rd] */
  int64_t ld_rd;
  const float* m;           /* [N][51] projected target distribution (asvrl_c51_project) */
  float grad_scale;         /* 1 / B */
  int32_t _pad1;
  float* loss;              /* [N] -sum m log softmax(q[a_b]) */
  /* saved activations (operand type, row-major, natural feature order): the weight-gradient inputs */
  void *xb, *f, *hv1, *ha1, *hv2, *ha2;   /* [N][32], [N][256], [N][128] x 4 */
  /* pre-activation gradients (operand type): dz of output_layer_v [N][64] (51 + zero pad), of
   * output_layer_a [N][1280] (1275 + zero pad), of the hidden layers [N][128] x 4, of the encoders [N][256] */
  void *dzv, *dza, *dz2v, *dz2a, *dz1v, *dz1a, *dzf;
} AsvRainbowNetIO;

/* Pack the encoders and composed noisy layers into AsvRainbowImgOut (one launch). */
int asvrl_rainbow_pack(const AsvRainbowSrc* src, const AsvRainbowImgOut* img, void* stream);
/* act_rainbow (agent.py:308-324) for every row: argmax_k sum softmax(q[k]) z, epsilon-greedy. */
int asvrl_rainbow_net_act(const AsvRainbowImg* w, const AsvRainbowNetIO* io, void* stream);

/* The window form of asvrl_rainbow_net_act (new entry points only: the ABI version stays 29). What it adds to the
 * pass: */
typedef struct AsvRainbowActEx {
  int32_t robots_per_env;  /* >= 1: row b belongs to env b / robots_per_env (env_mask) */
  int32_t _pad0;
  int64_t step_add;        /* the epsilon schedule and the exploration draw use *step_dev + step_add (step_dev NULL:
                              0 + step_add); unlike asvrl_rainbow_net_act the window form always draws */
  double* act_pair;        /* optional [N][2]: (action index, 0.0), what asvrl_env_step_ex takes with
                              is_continuous = 0 */
  double* rec_row;         /* optional [N][2]: the same pair, written only for rows of envs with env_mask != 0 */
  const uint8_t* env_mask; /* optional [N / robots_per_env]; NULL: every env */
  float* q_out;            /* optional [N][ld_q]: column k < 25 = Q[k] = sum_atoms p[k] z, the value act_rainbow takes
                              the arg-max of (agent.py:320); columns >= 25 are not written */
  int64_t ld_q;            /* >= 25 */
} AsvRainbowActEx;
/* io as asvrl_rainbow_net_act's, except that io->act_out may be NULL when ex->act_pair or ex->rec_row is given. The
 * images are whatever asvrl_rainbow_pack last packed: composed noisy weights (training mode) or, with the source
 * pointers at weight_mu / bias_mu, the eval-mode network (policy_local.eval()). With step_add = 0, no mask and no
 * q_out the action is asvrl_rainbow_net_act's, bit for bit. Rows >= N of the last tile write nothing. */
int asvrl_rainbow_net_act_ex(const AsvRainbowImg* w, const AsvRainbowNetIO* io, const AsvRainbowActEx* ex,
                             void* stream);
/* sizeof(AsvRainbowActEx) as compiled. */
int64_t asvrl_rainbow_act_ex_struct_size(void);
/* The double-Q argmax of train_Rainbow (agent.py:605-609): act_idx[row] = argmax_k Q[k]. */
int asvrl_rainbow_net_argmax(const AsvRainbowImg* w, const AsvRainbowNetIO* io, void* stream);
/* p(s', a*) of the target net (agent.py:610-612): p_out[row] = softmax(q[act_idx[row]]). */
int asvrl_rainbow_net_pick(const AsvRainbowImg* w, const AsvRainbowNetIO* io, void* stream);
/* The training pass of train_Rainbow (agent.py:613-636) on the online net: forward saving the
 * activations, loss_b = -sum m log softmax(q[a_b]), and the backward of grad_scale * sum_b w_b loss_b
 * down to the encoders' pre-activations (the weight gradients then come from asvrl_linear_wgrad_multi
 * over the saved activations / dz images, the encoders' by the fold). */
int asvrl_rainbow_net_train(const AsvRainbowImg* w, const AsvRainbowNetIO* io, void* stream);

/* ---------------------------------------------------------------- optimiser (agent.py) */

/* clip_grad_norm_(params, max_norm) followed by optim.Adam(lr, betas, eps).step() over one
 * flat f32 parameter buffer of n elements (agent.py:75-76,98 with the clips at
 * agent.py:415,426,471,636). grads are scaled in place by min(1, max_norm / (norm + 1e-6))
 * (max_norm <= 0: no clipping); *step (f32, device) is incremented before the bias
 * corrections are taken; norm_out (f32 device scalar, optional) receives the pre-clip global
 * norm that clip_grad_norm_ returns. work: >= 64 doubles of device scratch. Two launches,
 * no host synchronisation (capturable). */
int asvrl_adam_clip(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                    float* step, float lr, float beta1, float beta2, float eps, float max_norm,
                    float* norm_out, double* work, void* stream);

/* The second half of asvrl_adam_clip alone: clip + Adam with the squared norm given as nparts
 * f64 partial sums (asvrl_partial_sums_norm; every workgroup folds them in the same fixed order)
 * and *step already incremented. One launch. */
int asvrl_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                    const float* step, float lr, float beta1, float beta2, float eps, float max_norm,
                    float* norm_out, const double* norm_parts, int32_t nparts, void* stream);

/* asvrl_adam_step that also writes every updated parameter into the bf16 MFMA weight images (ABI v10;
 * replaces the asvrl_critic_pack / asvrl_mlp_pack / asvrl_iqn_pack launch after the step, same values).
 * Segment: the rows x cols row-major weight at params[flat_off...]; element (r, c) goes to image position
 * (row0 + r + q*rep_row, col0 + c + q*rep_col) for q < nrep, swapped if transposed; f32 = 1 writes
 * image[row] as f32 (a bias copy, cols = 1), otherwise the bf16 fragment image of K columns (chained = 1:
 * an accumulator-fed layer's order). counter (optional): incremented once by the launch. */
#define ASVRL_MAX_PACK_SEGS 16
typedef struct AsvPackSeg {
  int64_t flat_off;
  void* image;
  int32_t rows, cols, K, chained;
  int32_t transposed, f32, row0, col0;
  int32_t nrep, rep_row, rep_col, reserved;
} AsvPackSeg;
int asvrl_adam_step_pack(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                         const float* step, float lr, float beta1, float beta2, float eps, float max_norm,
                         float* norm_out, const double* norm_parts, int32_t nparts, const AsvPackSeg* segs,
                         int32_t nseg, int64_t* counter, void* stream);

/* Agent.soft_update (agent.py:643-679) on the device: target[i] <- tau * local[i] + (1 - tau) * target[i] over two
 * flat f32 buffers of n elements in the same order, and every new target[i] into the target's weight images through
 * the segment table, as asvrl_adam_step_pack does for the local ones (same segments, same values as the pack
 * launches). One launch, capturable. tau in (0, 1] and one_minus_tau are given as float(tau) and
 * float(1.0 - tau), the subtraction in double: the blend is fadd(fmul(tau, l), fmul(one_minus_tau, t)), two rounded
 * products and a rounded sum, never an FMA, which is bit for bit what torch gives for
 * TAU * l.data + (1.0 - TAU) * t.data. tau == 1 copies local[i] (a hard update: a non-finite target value does not
 * survive as NaN). counter (optional, i64 device scalar, read only) with interval > 0: the launch writes nothing
 * unless counter[0] % interval == 0; counter NULL or interval 0: unconditional. n == 0 returns 0. Errors (before
 * any launch, asvrl_last_error names the argument): target or local NULL, n < 0, nseg outside
 * 0..ASVRL_MAX_PACK_SEGS, segs NULL with nseg > 0, a segment outside [0, n), an image K that is not a multiple of
 * 16, interval < 0, tau outside (0, 1]. */
int asvrl_target_update_pack(float* target, const float* local, int64_t n, float tau, float one_minus_tau,
                             const int64_t* counter, int64_t interval, const AsvPackSeg* segs, int32_t nseg,
                             void* stream);

/* ---------------------------------------------------------------- Linear weight gradients */

/* grad_weight / grad_bias of an nn.Linear from bf16 activations over R rows (the backward's
 * dW = dZ^T X, db = dZ.sum(0), AC_IQN_model.py:398-404 layers): dw[m][k] = sum_r dz[r][m] x[r][k],
 * db[m] = sum_r dz[r][m] (db optional). dz (R x M, leading dim ldz) and x (R x K, ldx) are bf16
 * row-major, 16-byte aligned, ld multiples of 8; R a multiple of 32. (M, K) in {(256, 64),
 * (128, 256), (128, 128), (64, 64), (256, 32)}. accumulate = 0 overwrites dw/db, 1 adds. Deterministic
 * (fixed-order partial sums). work: asvrl_linear_wgrad_workspace(M, K) floats. */
int64_t asvrl_linear_wgrad_workspace(int32_t M, int32_t K);
int asvrl_linear_wgrad(const void* dz, int64_t ldz, const void* x, int64_t ldx, int32_t R, int32_t M,
                       int32_t K, float* dw, float* db, int32_t accumulate, float* work,
                       int64_t work_floats, void* stream);

/* The same without the final reduction: writes *groups_out partials of (M*K + M) floats each
 * into `partial` (asvrl_linear_wgrad_groups(R, M, K) of them); reduce later, possibly together
 * with other layers, with asvrl_partial_sums. */
int32_t asvrl_linear_wgrad_groups(int32_t R, int32_t M, int32_t K);
int asvrl_linear_wgrad_partial(const void* dz, int64_t ldz, const void* x, int64_t ldx, int32_t R, int32_t M,
                               int32_t K, float* partial, int64_t partial_floats, int32_t* groups_out,
                               void* stream);

/* Several layers' partials in ONE launch (ABI v9; replaces one partial launch per layer on side
 * streams joined back). Segment k writes groups_out[k] partials, bit-identical to its own launch
 * (same groups, same summation order):
 *   kind ASVRL_WGRAD_MFMA : asvrl_linear_wgrad_partial (bf16 dz, x); (M, K) in {(256, 64), (128, 256),
 *                           (128, 128), (256, 32), (32, 128)};
 *   kind ASVRL_WGRAD_VEC  : asvrl_linear_wgrad_vec_partial (dz = dq f32 with stride ldz, M = 1, K = 128);
 *   kind ASVRL_WGRAD_SMALL: asvrl_small_wgrad_partial (f32 dz, x; M | 256, K <= 4). */
#define ASVRL_MAX_WGRAD_SEGS 24
#define ASVRL_WGRAD_MFMA 0
#define ASVRL_WGRAD_VEC 1
#define ASVRL_WGRAD_SMALL 2
typedef struct AsvWgradSeg {
  const void* dz;
  int64_t ldz;
  const void* x;
  int64_t ldx;
  int32_t R, M, K, kind;
  float* partial;
  int64_t partial_floats;
} AsvWgradSeg;
int asvrl_linear_wgrad_multi(const AsvWgradSeg* segs, int32_t nseg, int32_t* groups_out, void* stream);

/* Every gradient of the Actor (AC_IQN_model.py:284-321) after asvrl_actor_backward, in ONE launch (ABI 19;
 * replaces asvrl_linear_wgrad_multi + asvrl_partial_sums_norm of agent.py:424-426's actor_loss.backward()):
 * hidden_layer / hidden_layer_2 weight and bias grads, output_layer's, the two observation encoders' (folded
 * from the 256 x 32 encoder image over the five object copies), the actor loss (sum of n_loss per-tile
 * partials), the squared-norm partials clip_grad_norm_ folds (asvrl_adam_step's norm_parts) and the Adam
 * step count (*step += 1). Each 32 x 32 output tile is reduced over S row splits by the split that arrives
 * last, in split order: deterministic, no partial buffer for another launch. Activations (operand dtype,
 * contiguous, 16-byte aligned): xb [B][32], h0 [B][256], h1, h2, dz2, dz1 [B][128], dz0 [B][256]; dout f32
 * [B][2]. Gradients f32, row-major as the nn.Linear parameters; enc_grad = self_w 56x7 | self_b 56 |
 * obj_w 40x5 | obj_b 40. work: asvrl_actor_grads_workspace(B) floats; counters:
 * asvrl_actor_grads_counters() ints, zero before the first launch (each launch leaves them zero). */
typedef struct AsvActorGradIO {
  const void* xb;
  const void* h0;
  const void* h1;
  const void* h2;
  const float* dout;
  const void* dz2;
  const void* dz1;
  const void* dz0;
  int32_t B, n_loss;
  const float* tile_loss;   /* optional (with loss_out) */
  float* loss_out;
  float* w1_grad;           /* hidden_layer [128][256], [128] */
  float* b1_grad;
  float* w2_grad;           /* hidden_layer_2 [128][128], [128] */
  float* b2_grad;
  float* wo_grad;           /* output_layer [2][128], [2] */
  float* bo_grad;
  float* enc_grad;          /* [688] */
  double* norm_parts;       /* optional: asvrl_actor_grads_norm_parts() slots */
  float* step;              /* optional */
  float* work;
  int64_t work_floats;
  int32_t* counters;
} AsvActorGradIO;
int64_t asvrl_actor_grads_workspace(int32_t B);
int32_t asvrl_actor_grads_counters(void);
int32_t asvrl_actor_grads_norm_parts(void);
int asvrl_actor_grads(const AsvActorGradIO* io, void* stream);

/* One output unit's version: dw[k] = sum_r dq[r*ldq] x[r][k], db = sum_r dq[r*ldq] with dq f32 and
 * x bf16 (R x K, ldx); K in {64, 128, 256}; work >= 256 * (K + 1) floats. */
int asvrl_linear_wgrad_vec(const float* dq, int64_t ldq, const void* x, int64_t ldx, int32_t R, int32_t K, float* dw,
                           float* db, int32_t accumulate, float* work, int64_t work_floats, void* stream);

int32_t asvrl_linear_wgrad_vec_groups(int32_t R);
int asvrl_linear_wgrad_vec_partial(const float* dq, int64_t ldq, const void* x, int64_t ldx, int32_t R,
                                   int32_t K, float* partial, int64_t partial_floats, int32_t* groups_out,
                                   void* stream);

/* One pending reduction: dw[i] (+)= sum_g partial[g][i] for i < nw, db likewise for the
 * trailing nb values of each group's (nw + nb)-float partial (db optional). A segment with
 * nw + nb == 1 (a scalar over many groups) is reduced by a whole workgroup. */
#define ASVRL_MAX_SUM_SEGS 24
#define ASVRL_SUM_PLAIN 0
/* The 256 x 32 encoder-image partials (asvrl_mlp_pack's block-structured image) folded straight
 * into the contiguous gradients [self_w 56x7 | self_b 56 | obj_w 40x5 | obj_b 40] at dw (688
 * floats, nw = 688, nb = 0): the object encoder's five copies are summed, in object order, after
 * each copy's own fixed-order group sum (bit-identical to asvrl_encoder_fold after a plain sum). */
#define ASVRL_SUM_FOLD_ENCODERS 1
typedef struct AsvPartialSum {
  const float* partial;
  float* dw;
  float* db;
  int32_t groups, nw, nb, accumulate;
  int32_t stride;   /* floats per group in partial; 0 = nw + nb */
  int32_t boff;     /* offset of the bias partials within a group; 0 = nw. With stride / boff a
                       32-row MFMA reduction can fill a layer of fewer rows (IQN's 25 actions) */
  int32_t mode;     /* ASVRL_SUM_PLAIN or ASVRL_SUM_FOLD_ENCODERS */
  int32_t norm;     /* 1: the outputs count towards the gradient norm (asvrl_partial_sums_norm) */
} AsvPartialSum;
/* Reduce up to ASVRL_MAX_SUM_SEGS pending partial sets in one launch (fixed order per output). */
int asvrl_partial_sums(const AsvPartialSum* segs, int32_t nseg, void* stream);

/* asvrl_partial_sums that also prepares the global gradient norm of the segments with norm = 1
 * for an asvrl_adam_step right after (replaces asvrl_adam_clip's norm pass when every gradient is
 * produced by this launch and no all-reduce follows): each working workgroup writes the f64 sum of
 * the squares of the outputs it wrote to its own slot of norm_parts (asvrl_partial_sums_norm_parts
 * slots), and *step is incremented. */
int asvrl_partial_sums_norm(const AsvPartialSum* segs, int32_t nseg, double* norm_parts, float* step,
                            void* stream);
int32_t asvrl_partial_sums_norm_parts(const AsvPartialSum* segs, int32_t nseg);

/* ---------------------------------------------------------------- per-row MLPs (actor, encoders) */

/* f32 parameters of one AC-IQN network's per-row layers (AC_IQN_model.py:254-262, 389-404):
 * self_encoder (56 x 7), object_encoder (40 x 5); for an Actor also hidden_layer (128 x 256) and
 * hidden_layer_2 (128 x 128); for a Critic also action_encoder (128 x 2). Unused entries NULL. */
typedef struct AsvMlpSrc {
  const float* self_w;
  const float* self_b;
  const float* obj_w;
  const float* obj_b;
  const float* w1;
  const float* w2;
  const float* ae_w;
} AsvMlpSrc;

/* Packed images the kernels read (filled by asvrl_mlp_pack, which writes through these
 * pointers) plus direct pointers to the remaining f32 parameters. */
typedef struct AsvMlpWeights {
  const void* enc_frag;   /* both encoders as one block-structured 256 x 32 bf16 image (16 KB) */
  const float* b_enc;     /* [256] their biases (written by the pack) */
  const void* w1_frag;    /* hidden_layer, chained order (64 KB)          (Actor) */
  const void* w2_frag;    /* hidden_layer_2 (32 KB)                        (Actor) */
  const void* w2t_frag;   /* hidden_layer_2^T (32 KB, backward)            (Actor) */
  const void* w1t_frag;   /* hidden_layer^T (64 KB, backward)              (Actor) */
  const float* b1;        /* hidden_layer.bias [128]                       (Actor) */
  const float* b2;        /* hidden_layer_2.bias [128]                     (Actor) */
  const float* wout;      /* output_layer.weight [2][128]                  (Actor) */
  const float* bout;      /* output_layer.bias [2]                         (Actor) */
  const void* ae_frag;    /* action_encoder as a 128 x 16 image (cols 2.. zero) (Critic) */
  const float* b_ae;      /* action_encoder.bias [128]                     (Critic) */
  float out_scale;        /* Actor.atan_scale = float32(2 / pi) */
} AsvMlpWeights;

/* Rows in / out of the MLP kernels. Observation rows are the packed ASVRL_OBS_DIM layout at
 * row stride ldx floats (40 for env observations, 88 for replay rows), 16-byte aligned. */
typedef struct AsvMlpIO {
  const float* x;
  int64_t ldx;
  const float* act;       /* ENCODE: actions [n] at stride lda (G = relu(W_ae a + b_ae)) */
  int64_t lda;
  int32_t n;
  float* F;               /* ENCODE out [n][256] */
  float* G;               /* ENCODE out [n][128] (optional) */
  void* xb;               /* ENCODE (optional) / TRAIN out: bf16 copy of obs columns 0..31 [n][32] */
  float* a_out;           /* FWD / TRAIN out: actions, stride ld_aout */
  int64_t ld_aout;
  double* a_out64;        /* ACT out: [n][2] f64 */
  float* pre;             /* TRAIN out / backward in: pre-atan outputs [n][2] */
  void* h0;               /* TRAIN out: bf16 [n][256] encoder output (hidden_layer input) */
  void* h1;               /* TRAIN out: bf16 [n][128] */
  void* h2;               /* TRAIN out: bf16 [n][128] */
  const float* dA;        /* backward in: dL/d(action) [n][2] */
  float* dout;            /* backward out: dL/d(output_layer pre-activation) [n][2] */
  void* dz2;              /* backward out: bf16 [n][128] hidden_layer_2 pre-activation grad */
  void* dz1;              /* backward out: bf16 [n][128] hidden_layer pre-activation grad */
  void* dz0;              /* backward out: bf16 [n][256] encoder pre-activation grad */
  const int64_t* step_dev;      /* ACT: device step counter (epsilon schedule, trainer.py:257-264) */
  double eps_steps_per_count;   /* timesteps per counter tick (= n_envs) */
  double eps_total, eps_fraction, eps_initial, eps_final;
  uint64_t seed;                /* ACT: Philox key of the exploration draws */
} AsvMlpIO;

/* Pack the bf16 images of `w` from the f32 parameters in `src` (one launch). */
int asvrl_mlp_pack(const AsvMlpSrc* src, const AsvMlpWeights* w, void* stream);
/* observation_processor (AC_IQN_model.py:284-308) -> F, and action_encoder -> G, per row. */
int asvrl_mlp_encode(const AsvMlpWeights* w, const AsvMlpIO* io, void* stream);
/* Actor.forward (AC_IQN_model.py:310-321). mode 1 = ACT (epsilon-greedy f64 actions,
 * agent.py:207-225), 2 = FWD (f32 actions), 3 = TRAIN (f32 actions + saved activations). */
int asvrl_actor_forward(const AsvMlpWeights* w, const AsvMlpIO* io, int32_t mode, void* stream);
/* The AC-IQN learn step's prologue in ONE launch (ABI 18): asvrl_replay_sample's draw of B rows and
 * their quantile fractions (uniform ring, replay_buffer.py:26-45; taus of AC_IQN_model.py:419), the local
 * Actor's TRAIN forward on s (agent.py:419-421; outputs in train_io, n = B) and the target Actor's FWD
 * on s' into na [B][2] (agent.py:397-398) -- bit-identical to the three separate launches. B must be a
 * multiple of 32. */
typedef struct AsvSampleArgs {
  const float* ring;            /* [capacity][ASVRL_TR_DIM] */
  int64_t capacity;
  const int64_t* ring_state;    /* {head, size} to sample against */
  uint64_t seed, counter;
  const uint64_t* counter_dev;  /* optional, added to counter */
  int64_t guard;                /* skip the oldest rows a concurrent push of <= guard rows may overwrite */
  int32_t B, tau_sets, tau_n, _pad0;
  float* out;                   /* [B][ASVRL_TR_DIM] sampled rows */
  float* taus;                  /* optional [tau_sets][B][tau_n] */
} AsvSampleArgs;
int asvrl_learn_prologue(const AsvSampleArgs* s, const AsvMlpWeights* actor, const AsvMlpIO* train_io,
                         const AsvMlpWeights* target_actor, float* na, void* stream);
/* Backward of the Actor from dA to every layer's pre-activation gradient (agent.py:425). */
int asvrl_actor_backward(const AsvMlpWeights* w, const AsvMlpIO* io, void* stream);
/* Fold the 256 x 32 encoder-image gradient (dw, db from asvrl_linear_wgrad) back onto
 * self_encoder / object_encoder weight and bias gradients (object rows summed over objects). */
int asvrl_encoder_fold(const float* dw, const float* db, float* self_w, float* self_b, float* obj_w,
                       float* obj_b, int32_t accumulate, void* stream);
/* dw[m][k] = sum_r dz[r][m] x[r][k], db[m] = sum_r dz[r][m] for f32 inputs with K <= 4 and
 * M | 256 (the critic action_encoder). work >= ceil(R / 32) * (M*K + M) floats. */
int asvrl_small_wgrad(const float* dz, int64_t ldz, const float* x, int64_t ldx, int32_t R, int32_t M,
                      int32_t K, float* dw, float* db, int32_t accumulate, float* work,
                      int64_t work_floats, void* stream);
int asvrl_small_wgrad_partial(const float* dz, int64_t ldz, const float* x, int64_t ldx, int32_t R,
                              int32_t M, int32_t K, float* partial, int64_t partial_floats,
                              int32_t* groups_out, void* stream);

/* ---------------------------------------------------------------- closed-loop policy rollout (ABI 28) */

/* The AC-IQN Actor driving asvrl_policy_rollout. */
typedef struct AsvPolicy {
  AsvMlpWeights w;                /* the actor's packed images (asvrl_mlp_pack) */
  const float* obs_in;            /* [NT][ASVRL_OBS_DIM] the observation step 0 acts on (16-byte aligned) */
  const int64_t* step_dev;        /* epsilon schedule / exploration key: step = *step_dev + t (NULL: 0 + t) */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;   /* as AsvMlpIO's */
  uint64_t seed;                  /* Philox key of the exploration draws */
  double* actions;                /* optional record [K][NT][2]: the action every robot slot was given */
} AsvPolicy;

/* K closed-loop steps in one launch: for t < ro->n_steps, the Actor's epsilon-greedy act on every robot row
 * (asvrl_actor_forward mode 1 with step = *step_dev + t: the same MFMA chain, the same Philox draw keyed by the
 * global row and that step) and then the env step of asvrl_env_rollout on those actions. Step 0 acts on
 * pi->obs_in, step t > 0 on the observation step t - 1 produced -- bit for bit the 2 K launches of act and
 * asvrl_env_step_ex it replaces. The Actor's weight images are staged once into the LDS of the workgroup that
 * owns an env group, beside its env-step arrays, its robots' observation rows and action pairs; one workgroup
 * per CU. ro->actions must be NULL (the policy supplies the actions); every other AsvRollout member, ctl, `last`
 * and launch mean what they mean to asvrl_env_rollout (ro->noise with noise_mode 0: recorded perception noise
 * under a live policy). ctl->is_continuous must be 1. An env that is masked or held takes no action and its rows
 * of pi->actions are not written: pre-fill them. pi->obs_in may be last->obs. The caller's step counter is only
 * read. Per-robot parameters, layout 2 and an env group whose arrays do not fit the LDS beside the weights run
 * K x (the act launch into a stream-ordered scratch, the single step, the record launches) instead. */
int asvrl_policy_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                         const AsvStepOut* last, const AsvRollout* ro, const AsvPolicy* pi,
                         const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
/* sizeof(AsvPolicy) as compiled. */
int64_t asvrl_policy_struct_size(void);

/* ---------------------------------------------------------------- auto-reset inside rollout windows (ABI 29) */

/* Episodes restart inside a K-step window. After step t has written its outputs and records, every stepping env
 * whose env_done the step set is reset by asvrl_env_reset's sampler (cfg, ctl->seed, the draws keyed at
 * reset_counter + t + *ctl->counter_dev) and observed by the masked do_dynamics = 0 pass (ctl's noise_mode and
 * seed, gamma 0, keyed at obs_counter + t + *ctl->counter_dev), which writes `last` (obs, obs64, obj_cnt, reward,
 * done, info: what asvrl_env_reset_observe writes) and, in the closed loop, the row the Actor reads at step t + 1.
 * The records of row t keep the step's values. Bit for bit the composed loop: per step the act (closed loop),
 * asvrl_env_step_ex at counter + t, then asvrl_env_reset_observe on last->env_done AND ctl->env_mask. */
typedef struct AsvAutoReset {
  AsvResetCfg cfg;
  uint64_t reset_counter, obs_counter;   /* + t (+ *ctl->counter_dev) */
  const float* obs_in;   /* open loop: [NT][ASVRL_OBS_DIM] the rows in front of step 0 (needed for obs_prev);
                            closed loop: NULL (pi->obs_in is used) */
  float* obs_prev;       /* optional record [K][NT][ASVRL_OBS_DIM]: row t is the observation every robot row of a
                            stepping env had in front of step t (row 0: obs_in; row t > 0: what step t - 1, or its
                            reset, left); rows of envs that do not step are not written */
  int32_t* pushed;       /* optional [K]: per step, the rows of stepping envs with obj_cnt >= 0 are ADDED (integer
                            atomics): the caller zeroes it */
  int32_t* resets;       /* optional [n_envs]: resets of every env in the window (zeroed by the call) */
} AsvAutoReset;

/* asvrl_env_rollout / asvrl_policy_rollout with the auto-reset above in the step loop (one launch; per-robot
 * parameters, layout 2 and a carve that does not fit run K x the single launches, the reset launches and a small
 * record launch, with the same results). Needs ctl->trainer_deactivate, last->env_done, Philox noise (noise_mode 1
 * or 2: recorded noise cannot cover a sampled reset) and no ro->hold_done; cfg's counts and the batch's max_robots /
 * max_obs / max_cores within asvrl_env_reset's tables (32 robots, 32 obstacles, 16 cores). Everything else is the
 * two calls' own contract. */
int asvrl_env_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                         const AsvStepOut* last, const AsvRollout* ro, const AsvAutoReset* ar,
                         const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
int asvrl_policy_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                            const AsvStepOut* last, const AsvRollout* ro, const AsvPolicy* pi,
                            const AsvAutoReset* ar, const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
/* sizeof(AsvAutoReset) as compiled. */
int64_t asvrl_autoreset_struct_size(void);

/* The replay push of a whole window in one call: the rows of K steps (row t * n + k of every array; actions
 * [K * n][action_ld] f64) go into the ring in step-major, then row order, rows with obj_cnt_next < 0 skipped --
 * the ring bytes and {head, size} of K calls of asvrl_replay_push_ex on rows t = 0..K-1. A block counts only inside
 * its own step and takes the step's base from the K per-step counts: `pushed` ([K], e.g. AsvAutoReset.pushed), or,
 * when it is NULL, a pre-pass of K blocks that counts them into `work`. work: zeroed int32[2 + K], left zeroed in
 * its first two. snap as asvrl_replay_push_ex; *counter_inc += counter_by. K * n <= capacity. */
int asvrl_replay_push_window(const float* obs_prev, const float* obs_next, const int8_t* obj_cnt_next,
                             const double* actions, int32_t action_dim, int64_t action_ld, const double* reward,
                             const uint8_t* done, int32_t n, int32_t K, const int32_t* pushed, float* ring,
                             int64_t capacity, int64_t* ring_state, int32_t* work, int64_t* snap,
                             int64_t* counter_inc, int64_t counter_by, void* stream);

/* ---------------------------------------------------------------- evaluation bookkeeping over rollout windows */

/* Trainer.evaluation's per-step bookkeeping (trainer.py:286-303) over the records of one hold_done window, folded
 * into state that is carried from window to window. For every env with ended == 0 and t = 0 .. steps_run[e] - 1:
 * each existing robot (slot < n_robots[e]) that is not deact adds pow(gamma, length) * reward to ret, dt * N to time
 * and pc * |TL| * dt * N + pc * |TR| * dt * N (left to right; the thrusts after the step) to energy; info
 * ASVRL_INFO_COLLISION / ASVRL_INFO_REACH_GOAL set outcome (2 / 1) and deact; then
 * end = length >= episode_limit || a robot collided at this step || every existing robot is deact; length += 1;
 * on end the env is marked ended and the window's later rows of that env are ignored (the rollout steps an env on
 * after a collision until all its robots are deactivated: ignoring those rows is the evaluation's end rule).
 * Rows t >= steps_run[e] are never read. alive[e] = !ended[e] is written for every env, ready to be the next
 * window's env_mask. One launch, no atomics; the caller zeroes the carried state before the first window. */
typedef struct AsvEvalMetrics {
  int32_t n_steps;         /* K >= 1, the window's rows */
  int32_t n_envs;          /* E >= 1 */
  int32_t max_robots;      /* 1..32; NT = n_envs * max_robots */
  int32_t episode_limit;   /* trainer.py:297: 1000 */
  double gamma;
  /* the window's records and the batch (read only) */
  const double*  reward;     /* [K][NT] */
  const uint8_t* info;       /* [K][NT] */
  const double*  rs;         /* [K][ASVRL_NUM_FIELDS][NT]; only the ASVRL_F_TL and ASVRL_F_TR planes are read */
  const int32_t* steps_run;  /* [E] */
  const int32_t* n_robots;   /* [E] */
  const double*  dt;         /* [NT] every robot row's own dt, N and power coefficient */
  const double*  N;          /* [NT] */
  const double*  pc;         /* [NT] */
  /* carried state (read and written) */
  int32_t* length;   /* [E] steps the evaluation counted */
  uint8_t* ended;    /* [E] */
  uint8_t* alive;    /* [E] written only: !ended */
  uint8_t* deact;    /* [NT] */
  uint8_t* outcome;  /* [NT] 0 running, 1 reached its goal, 2 collided */
  double*  ret;      /* [NT] */
  double*  time;     /* [NT] */
  double*  energy;   /* [NT] */
} AsvEvalMetrics;

int asvrl_eval_metrics(const AsvEvalMetrics* m, void* stream);
/* sizeof(AsvEvalMetrics) as compiled. */
int64_t asvrl_eval_metrics_struct_size(void);

/* The episode histories of Trainer.evaluation (trainer.py:347-365; env.py:262-269, 348-351) cut out of episode-long
 * rollout records: the records of every window of an evaluation kept time-major over T steps (row s of each array is
 * step s of the episode), and length[e] = L the evaluation's own length after the run (AsvEvalMetrics.length).
 *
 * asvrl_eval_history_count: for robot row e * max_robots + j with j < n_robots[e], d = the first step s < min(L, T)
 * with info ASVRL_INFO_COLLISION or ASVRL_INFO_REACH_GOAL, n_act = d + 1 when there is one and L otherwise;
 * counts[0][row] = n_act + 1 (trajectory rows), counts[1][row] = n_act (actions), counts[2][row] = L + 1
 * (observations). A slot beyond n_robots[e] gets three zeros. No info row at or behind L is read.
 *
 * asvrl_eval_history_pack: with offsets the exclusive scans of the three count planes, in one launch
 *   traj   [offsets[0][row] + k][13]  k = 0: rs0, k > 0: rs[k - 1]; the 13 values in wamv.py:191-193 order (x, y, theta,
 *                                      velocity_r, velocity, left_pos, right_pos, left_thrust, right_thrust)
 *   act    [offsets[1][row] + k][2]   actions[k]
 *   obs_out[offsets[2][row] + k][32]  k = 0: obs0, k > 0: obs[k - 1]; the first 32 floats of the packed row
 *   cnt_out[offsets[2][row] + k]      k = 0: cnt0, k > 0: obj_cnt[k - 1]
 * for k below the row's count: every robot's history contiguous, robots in batch order, time fastest. A block takes
 * ASVRL_HISTORY_ROW_TILE rows by ASVRL_HISTORY_STEP_TILE steps; the f64 planes and the counts go through an LDS tile
 * (read along rows, written along a robot's run), the observation rows are copied 128 bytes at a time. Nothing at
 * or behind a row's count is read; a destination index at or past its *_rows capacity is not written. No atomics. */
#define ASVRL_HISTORY_ROW_TILE 32
#define ASVRL_HISTORY_STEP_TILE 16
#define ASVRL_TRAJ_DIM 13          /* wamv.py:191-193 */
#define ASVRL_HISTORY_OBS_DIM 32   /* self 7 | objects 5 x 5 of the packed row */

typedef struct AsvEvalHistory {
  int32_t n_steps;      /* T >= 1: rows of info, rs, obs and obj_cnt */
  int32_t n_envs;       /* E >= 1 */
  int32_t max_robots;   /* 1..32; NT = n_envs * max_robots */
  int32_t act_steps;    /* >= 1: rows of actions (an action table may be shorter or longer than T) */
  const uint8_t* info;       /* [T][NT] (count) */
  const int32_t* length;     /* [E] (count) */
  const int32_t* n_robots;   /* [E] (count) */
  int32_t*       counts;     /* [3][NT] written by count, read by pack */
  const int64_t* offsets;    /* [3][NT] exclusive scans of counts (pack) */
  const double*  rs0;        /* [ASVRL_NUM_FIELDS][NT] the state in front of step 0 */
  const double*  rs;         /* [T][ASVRL_NUM_FIELDS][NT] */
  const double*  actions;    /* [act_steps][NT][2] */
  const float*   obs0;       /* [NT][ASVRL_OBS_DIM] the observation pass's rows (16-byte aligned) */
  const float*   obs;        /* [T][NT][ASVRL_OBS_DIM] (16-byte aligned) */
  const int8_t*  cnt0;       /* [NT] */
  const int8_t*  obj_cnt;    /* [T][NT] */
  double* traj;              /* [traj_rows][13] */
  double* act;               /* [act_rows][2]; may be NULL when act_rows == 0 */
  float*  obs_out;           /* [obs_rows][32] (16-byte aligned) */
  int8_t* cnt_out;           /* [obs_rows] */
  int64_t traj_rows, act_rows, obs_rows;   /* the sums of the three count planes */
} AsvEvalHistory;

int asvrl_eval_history_count(const AsvEvalHistory* h, void* stream);
int asvrl_eval_history_pack(const AsvEvalHistory* h, void* stream);
/* sizeof(AsvEvalHistory) as compiled, and ASVRL_HISTORY_STEP_TILE. */
int64_t asvrl_eval_history_struct_size(void);
int32_t asvrl_eval_history_step_tile(void);

/* Return-to-go and calibration of recorded return distributions, for one group of n_envs * max_robots = NT robot
 * rows over episode-long records of n_steps = T steps (new entry point only: the ABI version stays 29). z and tau
 * [T][NT][32] f32 are the 32 quantile samples and their fractions behind the decision robot row n took at step t;
 * reward [T][NT] f64; n_act [NT] i32 (plane 1 of asvrl_eval_history_count's counts, clamped to 0..T here): robot n
 * acted at steps 0..A-1, A = n_act[n]. Per robot row that exists (n % max_robots < n_robots[n / max_robots]; the
 * others' outputs are not written), all in f64:
 *   G_A = 0, G_t = reward[t][n] + gamma * G_{t+1} for t = A-1 .. 0       (g_plane[t][n], rows t >= A not written)
 *   u_t = #{ j : z[t][n][j] <= G_t } in 0..32,  pit[n][u_t] += 1                                   (pit [NT][33])
 *   pinball[n] = sum_t sum_j rho(tau[t][n][j], G_t - z[t][n][j]),  rho(tau, d) = d * (tau - (d < 0 ? 1 : 0))
 *   bias[n] = sum_t (mean_t - G_t),  mean_t = (1/32) sum_j z[t][n][j];  pred0[n] = mean_0 (0 when A = 0)
 *   g0[n] = G_0 (0 when A = 0),  steps[n] = A
 * The sums over j are a fixed butterfly over the 32 lanes of a step and the sums over t run t = 0, 1, ... in
 * order, in one lane: no atomics, the same bits from run to run and for every block size. */
typedef struct AsvEvalDistStats {
  int32_t n_steps, n_envs, max_robots;
  int32_t block;           /* threads per block of both launches: 0 = 256, else a multiple of 64 up to 1024 */
  double gamma;
  const float* z;
  const float* tau;
  const double* reward;
  const int32_t* n_act;
  const int32_t* n_robots; /* [n_envs] */
  double* g_plane;         /* [T][NT]: scratch of the call and, to the caller, the return-to-go plane */
  double* g0;              /* [NT] */
  double* pred0;           /* [NT] */
  int32_t* pit;            /* [NT][33] */
  double* pinball;         /* [NT] */
  double* bias;            /* [NT] */
  int32_t* steps;          /* [NT] */
} AsvEvalDistStats;
#define ASVRL_DIST_SAMPLES 32
int asvrl_eval_dist_stats(const AsvEvalDistStats* s, void* stream);
/* sizeof(AsvEvalDistStats) as compiled. */
int64_t asvrl_eval_dist_stats_struct_size(void);

/* ---------------------------------------------------------------- the reference's perception-noise streams */

/* One env step's perception noise drawn from every robot's own numpy.random.RandomState stream (wamv.py:5-40,
 * drawn at :466-468 and :493-495), continued on the device: the rows asvrl_env_step / asvrl_env_rollout take as
 * explicit noise (noise mode 0), [NT][O + R][5] f64 with NT = n_envs * max_robots, O = max_obs, R = max_robots.
 *
 * A stream is numpy's get_state() tuple: key (624 MT19937 words), pos (0..624), has_gauss and the cached gauss.
 * Robot i of env e (row e * R + i) draws iff env_mask[e] != 0 (a NULL mask: every env), i < n_robots[e] and
 * rflags[row] does not carry ASVRL_FLAG_DEACTIVATED; a robot that does not draw keeps its stream bit for bit and
 * gets a zero row. One that draws takes five values -- normal(0, pos_std) twice, normal(0, vel_std) twice,
 * vonmises(0, r_kappa), as Perception.draw_candidate_noise -- for every obstacle k < n_obs[e] into slot k and then
 * for every robot j < n_robots[e], j != i, not deactivated, into slot O + j (MarineNavEnv3._pack's order); every
 * other slot of the row is zero. pos_std, vel_std and r_kappa are those of the AsvParams argument, or of
 * robot_params[row] when the table is given (AsvEnvState.robot_params). The draws are numpy's word for word:
 * MT19937 words and every accept / reject decision of the normal's polar method exactly; the values through the
 * device's log / sqrt / cos / acos / fmod (asvrl_noise_streams) or the host's (asvrl_noise_streams_host).
 * draws_n / draws_sum / draws_sq (all three or none) accumulate the count, sum and sum of squares of the values
 * drawn, in draw order. One launch, one wave per robot row, no atomics. */
typedef struct AsvNoiseStreams {
  int32_t n_envs;      /* E >= 1 */
  int32_t max_robots;  /* R in 1..256 */
  int32_t max_obs;     /* O >= 0; (O + R) * 40 bytes of LDS per workgroup must fit (O + R <= 1024) */
  int32_t _pad0;
  /* the batch (read only) */
  const int32_t* n_robots;      /* [E] */
  const int32_t* n_obs;         /* [E] */
  const uint8_t* rflags;        /* [NT] */
  const uint8_t* env_mask;      /* [E] or NULL */
  const AsvParams* robot_params; /* [NT] or NULL: every robot AsvParams' pos_std / vel_std / r_kappa */
  /* the streams (read and written) */
  uint32_t* key;        /* [NT][624] */
  int32_t*  pos;        /* [NT] */
  int32_t*  has_gauss;  /* [NT] */
  double*   gauss;      /* [NT] */
  /* written */
  double*   noise_out;  /* [NT][O + R][5] */
  /* accumulated (all NULL: not counted) */
  int64_t*  draws_n;    /* [NT] */
  double*   draws_sum;  /* [NT] */
  double*   draws_sq;   /* [NT] */
} AsvNoiseStreams;

int asvrl_noise_streams(const AsvParams* p, const AsvNoiseStreams* ns, void* stream);
/* The same call on HOST pointers, run on the CPU by the same draw functions (csrc/asvrl_rs_stream.h): it needs no
 * GPU, and pins the algorithm to numpy bit for bit where the host's libm is numpy's. `stream` is ignored. */
int asvrl_noise_streams_host(const AsvParams* p, const AsvNoiseStreams* ns, void* stream);
/* sizeof(AsvNoiseStreams) as compiled. */
int64_t asvrl_noise_streams_struct_size(void);

/* ---------------------------------------------------------------- DQN (agent.py:271-287, 518-545)
 * DQN_Policy (DQN_model.py) has the Actor's trunk layer for layer (both observation encoders, hidden_layer,
 * hidden_layer_2) and a 128 -> A output layer (A = 25) without a squash. Its images are the Actor's
 * (AsvMlpWeights) plus the output layer padded to ASVRL_DQN_MAX_ACTIONS rows as one chained fragment image.
 * Columns >= A never enter a max, an arg-max or a gradient. New entry points only: the ABI version stays 29. */
#define ASVRL_DQN_MAX_ACTIONS 32
typedef struct AsvDqnWeights {
  AsvMlpWeights trunk;    /* wout: f32 output_layer.weight [A][128], bout: [A]; ae_frag, b_ae, out_scale unused */
  const void* head_frag;  /* output layer, 32 x 128 chained image, rows A.. zero (written by the pack) */
  int32_t n_actions;      /* A, 2..ASVRL_DQN_MAX_ACTIONS */
  int32_t _pad0;
} AsvDqnWeights;

/* Batched act: Q on n packed observation rows, arg-max (first maximum), epsilon-greedy with the linear
 * schedule on the device step counter (trainer.py:257-264): greedy iff random() > eps, else uniform over 0..A-1.
 * act_out[row * ld_act] = action index, act_out[row * ld_act + 1] = 0. */
typedef struct AsvDqnActIO {
  const float* x;         /* [n] rows of ASVRL_OBS_DIM at stride ldx floats, 16-byte aligned */
  int64_t ldx;
  int32_t n;
  int32_t _pad0;
  double* act_out;        /* f64 [n][ld_act], ld_act >= 2 */
  int64_t ld_act;
  float* q_out;           /* optional f32 [n][A]: the Q rows the arg-max was taken over */
  const int64_t* step_dev;      /* device step counter (NULL: step 0) */
  double eps_steps_per_count;   /* timesteps per counter tick (= n_envs) */
  double eps_total, eps_fraction, eps_initial, eps_final;
  uint64_t seed;                /* Philox key of the exploration draws */
} AsvDqnActIO;

/* One DQN gradient over B replay rows (ASVRL_TR_DIM layout: s | s' | action index | . | reward | done):
 * q = Q_local(s)[a], q_next = max_a Q_target(s'), y = r + (1 - d) gamma q_next, loss = mean smooth_l1(q - y)
 * (beta 1), dQ[b][a_b] = clamp(q - y, -1, 1) / B, and the backward to every layer's pre-activation gradient.
 * Saved activations and gradients are in the build's operand type (bf16 / f32). */
typedef struct AsvDqnGradIO {
  const float* rows;      /* [B] replay rows at stride ld_rows floats, 16-byte aligned */
  int64_t ld_rows;
  int32_t B;              /* a positive multiple of 32 */
  float gamma;
  void* xb;               /* out [B][32]: obs columns 0..31 of s (operand of the encoder weight gradient) */
  void* h0;               /* out [B][256] */
  void* h1;               /* out [B][128] */
  void* h2;               /* out [B][128] */
  float* q_sel;           /* out [B]: Q_local(s)[a] */
  float* q_next;          /* out [B]: max_a Q_target(s') */
  void* dz_out;           /* out [B][32]: dQ at column a, zero elsewhere */
  void* dz2;              /* out [B][128] */
  void* dz1;              /* out [B][128] */
  void* dz0;              /* out [B][256] */
  float* tile_loss;       /* out [B / 32]: per-tile loss partials, loss = their sum */
} AsvDqnGradIO;

/* The trunk images (as asvrl_mlp_pack) and the head image of `w` from the f32 parameters. */
int asvrl_dqn_pack(const AsvMlpSrc* src, const float* wout, const AsvDqnWeights* w, void* stream);
int asvrl_dqn_act(const AsvDqnWeights* w, const AsvDqnActIO* io, void* stream);
/* Two launches, no host sync: both forwards (local on s saving activations, target on s'), then loss + backward.
 * The weight gradients follow from (dz_out, h2), (dz2, h1), (dz1, h0), (dz0, xb) by asvrl_linear_wgrad_multi. */
int asvrl_dqn_grad(const AsvDqnWeights* local, const AsvDqnWeights* target, const AsvDqnGradIO* io, void* stream);
/* sizeof(AsvDqnWeights), sizeof(AsvDqnActIO), sizeof(AsvDqnGradIO) as compiled. */
int64_t asvrl_dqn_weights_struct_size(void);
int64_t asvrl_dqn_act_struct_size(void);
int64_t asvrl_dqn_grad_struct_size(void);

/* ---------------------------------------------------------------- closed-loop rollout windows for DQN
 * New entry points only: the ABI version stays 29. */

/* DQN_Policy driving asvrl_dqn_rollout. */
typedef struct AsvDqnPolicy {
  AsvDqnWeights w;                /* asvrl_dqn_pack's images */
  const float* obs_in;            /* [NT][ASVRL_OBS_DIM] the observation step 0 acts on (16-byte aligned) */
  const int64_t* step_dev;        /* epsilon schedule / exploration key: step = *step_dev + t (NULL: 0 + t) */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;   /* as AsvDqnActIO's */
  uint64_t seed;                  /* Philox key of the exploration draws */
  double* actions;                /* optional record [K][NT][2]: (action index, 0.0) of every robot slot */
} AsvDqnPolicy;

/* asvrl_policy_rollout and asvrl_policy_rollout_ar under DQN_Policy: for t < ro->n_steps, asvrl_dqn_act on every
 * robot row (the same MFMA chain, the first arg-max, the same Philox draw keyed by the global row and
 * step = *step_dev + t) and then the env step on the discrete action -- bit for bit the 2 K launches of
 * asvrl_dqn_act and asvrl_env_step_ex (and, with the auto-reset, asvrl_env_reset_observe) they replace. The
 * contract is the two Actor calls' word for word, except: ctl->is_continuous must be 0, pi->w.n_actions must be in
 * 2..ASVRL_DQN_MAX_ACTIONS and pi->w.head_frag must be non-null. The trunk's images are staged into LDS as the
 * Actor's are; the head's image and bias are read from L2. The caller's step counter is only read. Per-robot
 * parameters, layout 2 and an env group whose arrays do not fit the LDS beside the weights run K x (asvrl_dqn_act
 * into a stream-ordered scratch, the single step, the record launches and, with the auto-reset, the reset
 * launches) instead. */
int asvrl_dqn_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                      const AsvStepOut* last, const AsvRollout* ro, const AsvDqnPolicy* pi,
                      const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
int asvrl_dqn_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                         const AsvStepOut* last, const AsvRollout* ro, const AsvDqnPolicy* pi,
                         const AsvAutoReset* ar, const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
/* sizeof(AsvDqnPolicy) as compiled. */
int64_t asvrl_dqn_policy_struct_size(void);

/* ---------------------------------------------------------------- DDPG (agent.py:252-269, 478-516)
 * DDPG_model.Actor is the AC-IQN Actor layer for layer and runs its kernels unchanged. DDPG_model.Critic is one
 * scalar per sample: both observation encoders -> F (256), hidden_layer 256 -> 128 (h1), the product with
 * G = relu(action_encoder(a)), hidden_layer_2 128 -> 128 (h2) and a 128 -> 1 output. It runs the one-wave Actor
 * tile: its images are the Actor's (AsvMlpWeights, asvrl_mlp_pack) and the action encoder is read as f32.
 * New entry points only: the ABI version stays 29. */
typedef struct AsvDdpgWeights {
  AsvMlpWeights trunk;    /* enc / w1 / w2 images (w2t / w1t for a backward), b1, b2; wout: f32 [2][128], row 0
                             output_layer.weight, row 1 padding; bout: f32 [2], element 0 output_layer.bias;
                             ae_frag, b_ae, out_scale unused */
  const float* wae;       /* action_encoder weight, f32 [128][2] */
  const float* bae;       /* action_encoder bias, f32 [128] */
} AsvDdpgWeights;

/* One DDPG critic gradient over B replay rows (ASVRL_TR_DIM layout: s | s' | action (2) | reward | done):
 * q = Q_local(s, a), q_next = Q_target(s', na), y = r + gamma (1 - d) q_next, loss = mean smooth_l1(q - y)
 * (beta 1), dq = clamp(q - y, -1, 1) / B, and the backward to every layer's pre-activation gradient. Saved
 * activations and gradients are in the build's operand type (bf16 / f32) unless marked f32. */
typedef struct AsvDdpgGradIO {
  const float* rows;      /* [B] replay rows at stride ld_rows floats, 16-byte aligned */
  int64_t ld_rows;
  int32_t B;              /* a positive multiple of 32 */
  float gamma;
  const float* na;        /* [B] the target actor's action on s' at stride ld_na floats */
  int64_t ld_na;
  void* xb;               /* out [B][32]: obs columns 0..31 of s (operand of the encoder weight gradient) */
  void* h0;               /* out [B][256]: F */
  void* h1;               /* out [B][128] */
  void* p;                /* out [B][128]: h1 * G, hidden_layer_2's input */
  void* h2;               /* out [B][128] */
  float* q;               /* out f32 [B] */
  float* q_next;          /* out f32 [B] */
  float* dq;              /* out f32 [B]: the output layer's pre-activation gradient */
  void* dz2;              /* out [B][128] */
  void* dz1;              /* out [B][128] */
  float* dzG;             /* out f32 [B][128]: the action encoder's pre-activation gradient */
  void* dz0;              /* out [B][256]: dzF */
  float* tile_loss;       /* out f32 [B / 32]: per-tile loss partials, loss = their sum */
} AsvDdpgGradIO;

/* The actor step's gradient to the action (agent.py:504-507): q = Q_local(s, a_pi), loss = -mean q,
 * dA = d loss / d a_pi, in one launch without saved activations. */
typedef struct AsvDdpgActorIO {
  const float* x;         /* [B] observation rows at stride ldx floats, 16-byte aligned */
  int64_t ldx;
  const float* act;       /* [B] the actor's actions at stride lda floats */
  int64_t lda;
  int32_t B;              /* a positive multiple of 32 */
  int32_t _pad0;
  float* q;               /* optional out f32 [B] */
  float* dA;              /* out f32 [B][2] */
  float* tile_loss;       /* out f32 [B / 32]: per-tile partials of -mean q */
} AsvDdpgActorIO;

/* Two launches, no host sync: both forwards (local on (s, a) saving activations, target on (s', na)), then
 * loss + backward. The weight gradients follow from (dq, h2), (dz2, p), (dz1, h0), (dzG, a), (dz0, xb) by
 * asvrl_linear_wgrad_multi. */
int asvrl_ddpg_grad(const AsvDdpgWeights* local, const AsvDdpgWeights* target, const AsvDdpgGradIO* io, void* stream);
int asvrl_ddpg_actor_grad(const AsvDdpgWeights* local, const AsvDdpgActorIO* io, void* stream);
/* sizeof(AsvDdpgWeights), sizeof(AsvDdpgGradIO), sizeof(AsvDdpgActorIO) as compiled. */
int64_t asvrl_ddpg_weights_struct_size(void);
int64_t asvrl_ddpg_grad_struct_size(void);
int64_t asvrl_ddpg_actor_struct_size(void);

/* ---------------------------------------------------------------- SAC (agent.py:289-306, 547-595)
 * SAC_model.Critic is DDPG_model.Critic (AsvDdpgWeights, the one-scalar critic tile) twice. SAC_model.Actor is the
 * Actor's trunk under two 128 -> 2 heads: mu = Wmu h2 + bmu, ls = clamp(Wls h2 + bls, -20, 2), sigma = exp(ls),
 * z = mu + sigma eps, a = (2/pi) atan(z), logp = sum_d [-eps_d^2 / 2 - ls_d - log sqrt(2 pi) - log(1 - a_d^2 + 1e-6)]
 * (SAC_model.py:175-199). eps: an optional [n][2] f32 input used as is; NULL draws it in the kernel by Philox +
 * Box-Muller keyed by (row, counter, seed) in one of three streams (target actor, local actor, act) that never share
 * draws. The eps used is always written out. New entry points only: the ABI version stays 29. */
typedef struct AsvSacActorWeights {
  AsvMlpWeights trunk;    /* enc / w1 / w2 images (w2t / w1t for the backward), b1, b2, out_scale; wout: `head`,
                             bout: `bhead` (the Actor's staging reads their leading two rows); ae_frag, b_ae unused */
  const float* head;      /* f32 [4][128]: output_layer_mu.weight (rows 0, 1), output_layer_log_std.weight (2, 3) */
  const float* bhead;     /* f32 [4]: output_layer_mu.bias, output_layer_log_std.bias */
} AsvSacActorWeights;

/* Batched act (act_sac): greedy iff random() > eps_explore -- the sampled action -- else uniform per dimension; the
 * schedule and the greedy / uniform draw are asvrl_actor_forward's ACT mode, the noise counter is the step count. */
typedef struct AsvSacActIO {
  const float* x;         /* [n] rows of ASVRL_OBS_DIM at stride ldx floats, 16-byte aligned */
  int64_t ldx;
  int32_t n;
  int32_t _pad0;
  double* a_out64;        /* out [n][2] */
  const float* eps_in;    /* optional [n][2] */
  float* eps_out;         /* out [n][2]: the eps of the sampled action (also of rows that explore) */
  const int64_t* step_dev;   /* optional device step counter */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;   /* as AsvMlpIO's */
  uint64_t seed;
} AsvSacActIO;

/* The sampled actor over B replay rows, forward (asvrl_sac_actor_forward: the local actor on s saving what the
 * backward reads, the target actor on s') and backward (asvrl_sac_actor_backward). Saved activations and gradients
 * are in the build's operand type (bf16 / f32) unless marked f32. */
typedef struct AsvSacActorIO {
  const float* rows;      /* [B] replay rows at stride ld_rows floats, 16-byte aligned */
  int64_t ld_rows;
  int32_t B;              /* a positive multiple of 32 */
  float alpha;            /* entropy weight (backward) */
  const float* eps_local_in;    /* optional [B][2] */
  const float* eps_target_in;   /* optional [B][2] */
  uint64_t seed;
  uint64_t counter;             /* noise counter = counter + *counter_dev */
  const int64_t* counter_dev;   /* optional device counter (the learn counter) */
  void* xb;               /* out [B][32] */
  void* h0;               /* out [B][256] */
  void* h1;               /* out [B][128] */
  void* h2;               /* out [B][128] */
  float* mu;              /* out f32 [B][2] */
  float* ls;              /* out f32 [B][2]: log_std before the clamp */
  float* sigma;           /* out f32 [B][2] */
  float* z;               /* out f32 [B][2] */
  float* a;               /* out f32 [B][2]: a_pi */
  float* eps;             /* out f32 [B][2] */
  float* logp;            /* out f32 [B] */
  float* na;              /* out f32 [B][2]: the target actor's sampled action on s' */
  float* logp_next;       /* out f32 [B] */
  float* eps_next;        /* out f32 [B][2] */
  /* backward */
  const float* dA;        /* f32 [2][B][2]: each critic's share of d(-Qmin)/da (asvrl_sac_actor_grad); summed here */
  const float* q_pi;      /* f32 [2][B]: Q1, Q2(s, a_pi) */
  float* dhead;           /* out f32 [4][B]: dmu (rows 0, 1), dls (2, 3): the head's pre-activation gradients */
  void* dz2;              /* out [B][128] */
  void* dz1;              /* out [B][128] */
  void* dz0;              /* out [B][256] */
  float* tile_loss;       /* out f32 [B / 32]: per-tile partials of mean(alpha logp - min(Q1, Q2)) */
} AsvSacActorIO;

/* The twin critic gradient over B replay rows: c[k] is critic k's AsvDdpgGradIO (the same rows, ld_rows, B, gamma,
 * na and ld_na in both; every buffer its own). q_k = Q_k(s, a), q_next_k = Q_k_target(s', na),
 * y = r + gamma (1 - d) (min(q_next_1, q_next_2) - alpha logp_next), loss_k = mean (q_k - y)^2,
 * dq_k = 2 (q_k - y) / B, and each critic's backward as asvrl_ddpg_grad's. */
typedef struct AsvSacGradIO {
  AsvDdpgGradIO c[2];
  const float* logp_next; /* f32 [B]: the target actor's log-probability on s' */
  float* y;               /* optional out f32 [B]: the target */
  float alpha;
  int32_t _pad0;
} AsvSacGradIO;

/* The actor step's gradient to the action through both critics: q_pi[k] = Q_k(s, a_pi), and
 * dA[k] = w_k d(-Q_k)/da with w_k = 1 where Q_k is the smaller, 1/2 on an exact tie, 0 otherwise (torch.min). */
typedef struct AsvSacActorGradIO {
  const float* x;         /* [B] observation rows at stride ldx floats, 16-byte aligned */
  int64_t ldx;
  const float* act;       /* [B] a_pi at stride lda floats */
  int64_t lda;
  int32_t B;              /* a positive multiple of 32 */
  int32_t _pad0;
  float* q_pi;            /* out f32 [2][B] */
  float* dA;              /* out f32 [2][B][2] */
} AsvSacActorGradIO;

/* act_sac on n rows, one launch. */
int asvrl_sac_act(const AsvSacActorWeights* w, const AsvSacActIO* io, void* stream);
/* One launch: blockIdx.y = 0 the local actor on s, 1 the target actor on s'. */
int asvrl_sac_actor_forward(const AsvSacActorWeights* local, const AsvSacActorWeights* target, const AsvSacActorIO* io,
                            void* stream);
/* Two launches, no host sync: the four forwards (local 1, 2 on (s, a) saving activations, target 1, 2 on
 * (s', na)), then both losses + backwards. */
int asvrl_sac_grad(const AsvDdpgWeights* local1, const AsvDdpgWeights* local2, const AsvDdpgWeights* target1,
                   const AsvDdpgWeights* target2, const AsvSacGradIO* io, void* stream);
/* Two launches: q_pi of both critics, then each critic's weighted action gradient. */
int asvrl_sac_actor_grad(const AsvDdpgWeights* local1, const AsvDdpgWeights* local2, const AsvSacActorGradIO* io,
                         void* stream);
/* One launch: the head's backward from dA, the saved z / a / eps / ls / sigma and alpha, then dz2, dz1, dz0, the
 * actor-loss partials and dhead. */
int asvrl_sac_actor_backward(const AsvSacActorWeights* w, const AsvSacActorIO* io, void* stream);
/* sizeof of the five SAC structs as compiled. */
int64_t asvrl_sac_actor_weights_struct_size(void);
int64_t asvrl_sac_act_struct_size(void);
int64_t asvrl_sac_actor_struct_size(void);
int64_t asvrl_sac_grad_struct_size(void);
int64_t asvrl_sac_actor_grad_struct_size(void);

/* ---------------------------------------------------------------- closed-loop rollout windows for SAC
 * New entry points only: the ABI version stays 29. */

/* SAC's sampled actor driving asvrl_sac_rollout. */
typedef struct AsvSacPolicy {
  AsvSacActorWeights w;           /* the actor's images and its f32 head */
  const float* obs_in;            /* [NT][ASVRL_OBS_DIM] the observation step 0 acts on (16-byte aligned) */
  const int64_t* step_dev;        /* epsilon schedule, exploration and noise key: step = *step_dev + t (NULL: 0 + t) */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;   /* as AsvSacActIO's */
  uint64_t seed;                  /* Philox key of the exploration draws and of the action noise */
  double* actions;                /* optional record [K][NT][2]: the action every robot slot was given */
  int32_t deterministic;          /* != 0: eps = 0, nothing drawn: z = mu, the mean action (the epsilon schedule
                                     still applies) */
  int32_t _pad0;
} AsvSacPolicy;

/* asvrl_policy_rollout and asvrl_policy_rollout_ar under SAC's actor: for t < ro->n_steps, asvrl_sac_act on every
 * robot row (the same MFMA chain and f32 head, the noise of stream "act" keyed by the global row, step =
 * *step_dev + t and pi->seed, the same exploration draw) and then the env step on the action -- bit for bit the 2 K
 * launches of asvrl_sac_act (eps_in NULL; an all-zero eps_in with pi->deterministic) and asvrl_env_step_ex (and,
 * with the auto-reset, asvrl_env_reset_observe) they replace. The contract is the two Actor calls' word for word,
 * except: pi->w.head and pi->w.bhead must be non-null. The trunk's images are staged into LDS as the Actor's are,
 * and the head's 2 KB beside them. The caller's step counter is only read. Per-robot parameters, layout 2 and an
 * env group whose arrays do not fit the LDS beside the weights run K x (asvrl_sac_act into a stream-ordered
 * scratch, the single step, the record launches and, with the auto-reset, the reset launches) instead. */
int asvrl_sac_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                      const AsvStepOut* last, const AsvRollout* ro, const AsvSacPolicy* pi,
                      const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
int asvrl_sac_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                         const AsvStepOut* last, const AsvRollout* ro, const AsvSacPolicy* pi,
                         const AsvAutoReset* ar, const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
/* sizeof(AsvSacPolicy) as compiled. */
int64_t asvrl_sac_policy_struct_size(void);

/* ---------------------------------------------------------------- closed-loop rollout windows for IQN
 * New entry points only: the ABI version stays 29. */

/* IQN_Policy (act_iqn) driving asvrl_iqn_rollout. */
typedef struct AsvIqnPolicy {
  AsvCriticWeights w;             /* asvrl_iqn_pack's trunk images and the f32 encoders */
  AsvIqnHead head;                /* the padded output head and its bias */
  const float* obs_in;            /* [NT][ASVRL_OBS_DIM] the observation step 0 acts on (16-byte aligned) */
  const int64_t* step_dev;        /* tau draw, epsilon schedule and exploration key: step = *step_dev + t (NULL: 0 + t) */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;   /* as AsvIqnIO's */
  uint64_t seed;                  /* Philox key of the tau and exploration draws */
  double* actions;                /* optional record [K][NT][2]: (action index, 0.0) of every robot slot */
  float cvar;                     /* in (0, 1]: act_iqn's risk distortion, every tau times cvar (1: risk neutral) */
  int32_t _pad0;
} AsvIqnPolicy;

/* The closed loop under IQN_Policy: for t < ro->n_steps, asvrl_iqn_act on every robot row (K = 32 taus per state
 * drawn in the kernel on (row, *step_dev + t, seed), times cvar; the first arg-max of the mean; the epsilon-greedy
 * draw) and then the env step on the discrete action -- bit for bit the 2 K launches of asvrl_iqn_act and
 * asvrl_env_step_ex (and, with the auto-reset, asvrl_env_reset_observe) they replace. The act is NOT fused into the env
 * kernel (its 150 KB LDS image and its 16 waves per CU do not fit beside the env's carve): every layout runs, per
 * step, one asvrl_iqn_act_ex launch (step_add = t; it writes the step's action pairs and the record row itself), the
 * single step, the record launch and, with the auto-reset, the reset launches, all enqueued by this one call with
 * no host synchronisation. The contract is the two DQN calls' otherwise: ctl->is_continuous must be 0, ro->actions
 * null; pi->head.n_actions in 1..ASVRL_IQN_MAX_ACTIONS, pi->cvar in (0, 1]. The caller's step counter is only read. */
int asvrl_iqn_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                      const AsvStepOut* last, const AsvRollout* ro, const AsvIqnPolicy* pi,
                      const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
int asvrl_iqn_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                         const AsvStepOut* last, const AsvRollout* ro, const AsvIqnPolicy* pi,
                         const AsvAutoReset* ar, const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
/* sizeof(AsvIqnPolicy) as compiled. */
int64_t asvrl_iqn_policy_struct_size(void);

/* The two IQN windows under a per-robot risk level: every step's act launch is asvrl_iqn_act_risk. risk->cvar_rows is
 * per robot slot [NT] and constant over the window; the adaptive level is computed at every step from the row the
 * robot acts on. pi->cvar must be 1; risk->cvar_out is not used. pi->actions records (action index, level used); the
 * env step still takes (index, 0.0). */
int asvrl_iqn_rollout_risk(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                           const AsvStepOut* last, const AsvRollout* ro, const AsvIqnPolicy* pi,
                           const AsvIqnRisk* risk, const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
int asvrl_iqn_rollout_risk_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                              const AsvStepOut* last, const AsvRollout* ro, const AsvIqnPolicy* pi,
                              const AsvIqnRisk* risk, const AsvAutoReset* ar,
                              const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);

/* ---------------------------------------------------------------- closed-loop rollout windows for Rainbow
 * New entry points only: the ABI version stays 29. */

/* Rainbow_Policy (act_rainbow) driving asvrl_rainbow_rollout. */
typedef struct AsvRainbowPolicy {
  AsvRainbowImg w;                /* asvrl_rainbow_pack's images: noisy (training mode) or mu only (eval mode); the
                                     transposed images are not read */
  const float* support;           /* [51] */
  const float* obs_in;            /* [NT][ASVRL_OBS_DIM] the observation step 0 acts on (16-byte aligned) */
  const int64_t* step_dev;        /* epsilon schedule and exploration key: step = *step_dev + t (NULL: 0 + t) */
  double eps_steps_per_count, eps_total, eps_fraction, eps_initial, eps_final;   /* as AsvRainbowNetIO's */
  uint64_t seed;                  /* Philox key of the exploration draw */
  double* actions;                /* optional record [K][NT][2]: (action index, 0.0) of every robot slot */
} AsvRainbowPolicy;

/* The closed loop under Rainbow_Policy: for t < ro->n_steps, asvrl_rainbow_net_act on every robot row (the first
 * arg-max of Q[k] = sum_atoms p[k] z; the epsilon-greedy draw on (row, *step_dev + t, seed)) and then the env step on
 * the discrete action -- bit for bit the 2 K launches of asvrl_rainbow_net_act and asvrl_env_step_ex (and, with the
 * auto-reset, asvrl_env_reset_observe) they replace. As for IQN the act is NOT fused into the env kernel (the env
 * kernel is one f64 lane per robot-candidate pair with its own LDS layout, the network tile 4 MFMA waves per 32
 * rows): every layout runs, per step, one asvrl_rainbow_net_act_ex launch (step_add = t; it writes the step's action
 * pairs and the record row itself), the single step, the record launch and, with the auto-reset, the reset
 * launches, all enqueued by this one call with no host synchronisation (graph-capturable). The contract is the two
 * IQN calls' otherwise: ctl->is_continuous must be 0, ro->actions null. The caller's step counter is only read. */
int asvrl_rainbow_rollout(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                          const AsvStepOut* last, const AsvRollout* ro, const AsvRainbowPolicy* pi,
                          const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
int asvrl_rainbow_rollout_ar(const AsvParams* params, const AsvEnvState* state, const AsvStepCtl* ctl,
                             const AsvStepOut* last, const AsvRollout* ro, const AsvRainbowPolicy* pi,
                             const AsvAutoReset* ar, const AsvEnvLaunch* launch /* NULL: automatic */, void* stream);
/* sizeof(AsvRainbowPolicy) as compiled. */
int64_t asvrl_rainbow_policy_struct_size(void);

/* ---------------------------------------------------------------- misc */
const char* asvrl_last_error(void);
int asvrl_abi_version(void);
/* Bytes per learner-kernel operand element: 2 in libasvrl.so (bf16 MFMA operands, weight images
 * and saved activations, f32 accumulation), 4 in libasvrl_f32.so -- the same sources built with
 * ASVRL_OPERAND_F32=1, every operand f32 (v_mfma_f32_32x32x2_f32), the parity build of the
 * hand-written learner. Every other entry point is identical in both libraries. */
int32_t asvrl_operand_bytes(void);
/* sizeof(AsvParams, AsvEnvState, AsvStepCtl, AsvStepOut, AsvResetCfg) as compiled, for
 * binding checks (host pointer to 5 int64). */
void asvrl_struct_sizes(int64_t* out5);
/* ABI 27: sizeof(AsvRollout) as compiled (asvrl_struct_sizes keeps its five: its callers pass five slots). */
int64_t asvrl_rollout_struct_size(void);

#ifdef __cplusplus
}
#endif
#endif /* ASVRL_H */
