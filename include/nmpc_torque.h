/* nmpc_torque.h -- C-ABI of the torque layer: batched inverse dynamics + PD for the
 * plans the NMPC solve produces, and the forward dynamics that turn a torque or a PD target back into
 * motion under given contact forces or on a declared ground-contact law (libnmpc_hip.so).
 *
 * Replaces, for B robots at once:
 *   QuadrupedDynamics.id_torques            mpc_controller/utils/dynamics.py:136-163
 *       tau = pin.rnea(model, data, q, v, a)[-nu:]  -  sum_feet f_ee @ J_ee[:3, -nu:]
 *       (J_ee in LOCAL_WORLD_ALIGNED axes: f_ee is a world-frame force at the foot point)
 *   LocomotionMPC._compute_pd_torques       mpc_controller/mpc.py:592-599
 *       tau_pd = tau_ff + Kp (q_plan[-nu:] - q[-nu:]) + Kd (v_plan[-nu:] - v[-nu:])
 *   the recorded action                     DAgger/utils/RolloutMPC.py:228-250
 *       action = (tau + kd v_j) / kp + q_j       (the PD target that reproduces tau), joints re-ordered
 * The robot is a tree of 1-DoF joints with q_dot = v -- the reference's state
 * [px, py, pz, yaw, pitch, roll, joints] (dynamics.py:146-148) is three prismatic and three revolute
 * virtual joints in front of the legs.  The reference builds its model from a URDF through pinocchio
 * (both absent here); this boundary takes the same information as arrays.
 * All batch tensors are fp32 device pointers, row-major [batch][...]; calls are stream-ordered, never
 * allocate and never synchronise (the one exception is stated at nmpc_policy_rollout_batch).  Return values: NMPC_OK /
 * NMPC_E_* of nmpc.h. */
#ifndef NMPC_TORQUE_H
#define NMPC_TORQUE_H

#ifdef __cplusplus
extern "C" {
#endif

#define NMPC_TREE_MAX_JOINTS 32
#define NMPC_TREE_MAX_FEET 8

/* Host arrays, copied by nmpc_torque_create.  Joint i: parent[i] < i (-1 = world); type 0 revolute,
 * 1 prismatic; unit axis in the joint's own frame; fixed placement of the joint frame in the parent
 * frame, x_parent = R x_joint + p, as 12 floats (R row-major, then p); the body it carries: mass,
 * centre of mass, inertia about the centre of mass in body axes (xx, xy, xz, yy, yz, zz). */
typedef struct {
    int n_joints;             /* generalised coordinates, <= NMPC_TREE_MAX_JOINTS                  */
    int n_actuated;           /* nu: torques of the LAST n_actuated joints are returned            */
    int n_feet;               /* <= NMPC_TREE_MAX_FEET                                             */
    const int *parent;        /* [n_joints]                                                        */
    const int *type;          /* [n_joints]                                                        */
    const float *axis;        /* [n_joints][3]                                                     */
    const float *placement;   /* [n_joints][12]                                                    */
    const float *mass;        /* [n_joints]                                                        */
    const float *com;         /* [n_joints][3]                                                     */
    const float *inertia;     /* [n_joints][6]                                                     */
    const int *foot_joint;    /* [n_feet] joint whose body carries the foot                        */
    const float *foot_offset; /* [n_feet][3] foot point in that body's frame                       */
    float gravity[3];         /* world frame, e.g. {0, 0, -9.81}                                   */
} nmpc_tree_model;

int nmpc_torque_create(const nmpc_tree_model *model, int device_id, void **handle);
void nmpc_torque_destroy(void *handle);
const char *nmpc_torque_last_error(void *handle);

/* id_torques: q, v, a [B][n_joints]; f [B][n_feet][3] (world frame; NULL = no contact forces);
 * tau [B][n_actuated]. */
int nmpc_id_torques_batch(void *handle, int B, const float *q, const float *v, const float *a,
                          const float *f, float *tau, void *stream);

/* Forward dynamics: a = M(q)^-1 ( S^T tau - h(q, v) + sum_feet J_foot^T f ), the inverse of nmpc_id_torques_batch
 * (articulated-body algorithm, one thread per robot; contact forces are inputs, there is no contact model).
 * q, v [B][n_joints]; tau [B][n_actuated], the generalised forces of the LAST n_actuated joints, all other joints
 * carry none (NULL = all zero); f [B][n_feet][3] world frame (NULL = none); a [B][n_joints].
 * A robot whose elimination meets a joint pivot that is not a positive finite number (a massless leaf body) gets a
 * row of NaN, as nmpc_gather_rows marks its rows; the call returns NMPC_OK. */
int nmpc_fd_accel_batch(void *handle, int B, const float *q, const float *v, const float *tau,
                        const float *f, float *a, void *stream);

/* n_sub semi-implicit Euler substeps of length dt under constant f, the PD law re-evaluated every substep:
 *   tau = tau_ff + kp (q_des - q[-nu:]) - kd v[-nu:]     (q_des NULL: tau = tau_ff; tau_ff NULL = 0)
 *   a = fd(q, v, tau, f);  v += dt a;  q += dt v          (q_dot = v holds for this state)
 * q_des [B][n_actuated] is a recorded action in joint order (RolloutMPC.py:250).  q_out, v_out [B][n_joints] may
 * alias q, v; a_out [B][n_joints] (NULL allowed) is the acceleration of the last substep.  One launch per call.
 * NMPC_E_ARG (text in nmpc_torque_last_error): n_sub < 1, dt <= 0, a NULL q, v, q_out or v_out.  NaN rows as above. */
int nmpc_fd_step_batch(void *handle, int B, int n_sub, float dt, const float *q, const float *v,
                       const float *tau_ff, const float *q_des, float kp, float kd, const float *f,
                       float *q_out, float *v_out, float *a_out, void *stream);

/* The tree's inertia at q, from one composite-rigid-body pass (one thread per robot): the joint-space mass matrix M(q) of
 *   tau = M(q) a + h(q, v) - sum_feet J_foot^T f, so that column j of M is nmpc_id_torques_batch(q, 0, e_j) - (q, 0, 0) on a
 * tree with every joint actuated.  Any tree the handle accepts.  Massless bodies add nothing (a tree of them has M = 0); nothing
 * is inverted, so there are no NaN rows of the nmpc_fd_accel_batch kind: a q that is not finite gives outputs that are not
 * finite in its own row only.  M[i][j] of two joints that are not on one path to the root is written as 0.
 * NMPC_E_ARG (text in nmpc_torque_last_error), before any launch: B < 0, a NULL q or M. */
/* M [B][n_joints][n_joints], symmetric, every entry written. */
int nmpc_mass_matrix_batch(void *handle, int B, const float *q, float *M, void *stream);

/* The centre of mass of the whole tree and its centroidal momentum (pin.computeCentroidalMomentum of the articulated model:
 * the momentum of all bodies, linear and angular about the centre of mass, in world axes) with its map A_g(q).
 * NMPC_E_ARG, before any launch: B < 0, a NULL q, all outputs NULL, h without v, a tree whose total mass is zero (its centre
 * of mass is undefined; decided from the model of nmpc_torque_create). */
/* com [B][3] world; h [B][6] = [linear (world axes); angular about the centre of mass (world axes)] -- the slot order of
 * model 2's h; Ag [B][6][n_joints] with h = Ag v.  Every output may be NULL, not all; v may be NULL only if h is. */
int nmpc_centroidal_batch(void *handle, int B, const float *q, const float *v, float *com, float *h, float *Ag, void *stream);

/* How that momentum moves with q (pin.computeCentroidalDynamicsDerivatives' dh_dq, and the bias part of
 * pin.computeCentroidalMomentumTimeVariation): what a linearisation of h - A_g(q) v needs beside A_g and com.  One thread per
 * robot, one launch, three passes over the tree in world-frame spatial vectors about a point O at the robot (the origin of the
 * first frame that carries mass; nothing is taken through the world origin, so the base position does not cost accuracy):
 *   d h_O / d q_j = S_j x* h^c_j  -  I^c_j (S_j x v_p(j))           at fixed v
 * with S_j the motion axis of joint j, h^c_j, I^c_j the momentum and inertia of the subtree of body j, v_p(j) the velocity of the
 * parent body (zero for a root), x / x* the motion / force cross product; then
 *   d com / d q_j = lin(I^c_j S_j) / m                               (column j of Ag's linear rows over the total mass)
 *   d k_G / d q_j = d k_O / d q_j - d com / d q_j x l - (com - O) x d l / d q_j
 *   hdot_bias     = sum_j dh_dq[:, j] v_j  in joint order            (q_dot = v), so that h_dot = Ag a + hdot_bias.
 * Any tree the handle accepts; nothing is inverted, so a q or v that is not finite gives outputs that are not finite in its own
 * row only, and massless bodies add nothing.  Every entry of every given output is written.
 * NMPC_E_ARG, before any launch: B < 0, a NULL q or v, all outputs NULL, a tree whose total mass is zero. */
/* q, v [B][n_joints]; dh_dq [B][6][n_joints] = d(A_g(q) v)/dq_j, rows in the slot order of h; dcom_dq [B][3][n_joints];
 * hdot_bias [B][6].  Every output may be NULL, not all. */
int nmpc_centroidal_derivatives_batch(void *handle, int B, const float *q, const float *v,
                                      float *dh_dq, float *dcom_dq, float *hdot_bias, void *stream);

/* The centroidal momentum of a plant state alone: what a measured state's x0 carries in model 2's momentum slots when the solve
 * runs the articulated momentum model (nmpc_wb_set_state_momentum of nmpc.h).  One thread per state runs the outward pass of the
 * call above -- frame rotations, origins from the anchor point O, body velocities, every body's momentum about O, the totals, the
 * centre of mass -- and nothing else: no inward pass and no columns, 18 floats of LDS per joint and state, no scratch.  Rows are
 * strided, so the call reads a table of states and writes into the solver's tensors where they lie.  It agrees with
 * nmpc_centroidal_batch's h to fp32 rounding (another algorithm: not bit for bit) and, like the derivatives, does not see the
 * base position.  Any tree the handle accepts; a q or v that is not finite gives an h that is not finite in its own row only.
 * NMPC_E_ARG (text in nmpc_torque_last_error), before any launch: B < 0, a NULL q, v or h, qv_stride < n_joints, h_stride < 6,
 * h2 with h2_stride < 6, a tree whose total mass is zero. */
/* h = A_g(q) v of the articulated tree for B plant states: [linear; angular about the centre of mass], world axes,
 * model 2's slot order.  q, v at q + b*qv_stride (floats, >= n_joints); written to h + b*h_stride and, if h2 is
 * given, to h2 + b*h2_stride (strides >= 6).  skip: NULL, or dev int[B]; a row with skip[b] & skip_mask != 0 is
 * neither read nor written. */
int nmpc_state_momentum_batch(void *handle, int B, const float *q, const float *v, int qv_stride,
                              float *h, int h_stride, float *h2, int h2_stride,
                              const int *skip, int skip_mask, void *stream);

/* The ground-contact plant [decl] (the reference's is MuJoCo).  The ground is the plane z = ground_z with normal e_z.  A foot
 * point at world position p with world velocity pd and penetration delta = ground_z - p_z is pushed with
 *   f_z  = stiffness delta max(0, 1 - damping pd_z)  for delta > 0, else 0    (Hunt-Crossley: continuous at touch-down, never pulls)
 *   f_xy = -mu f_z pd_xy / sqrt(|pd_xy|^2 + slip_velocity^2)                  (regularised Coulomb, |f_xy| < mu f_z)
 * and the PD torque of the step is clamped to [-tau_max, tau_max] (tau_max <= 0: no limit).  The step integrates explicitly,
 * and both terms are dampers on the foot, so it is stable only while
 *   mu f_z dt / (slip_velocity m_foot) < 2   and   stiffness delta damping dt / m_foot < 2
 * (m_foot: the mass the foot point moves, a few hundred grams on the quadruped).  k = 1e4 N/m, c = 3 s/m, mu = 0.8,
 * slip_velocity = 0.05 m/s at dt = 0.5 ms let the 15 kg quadruped stand; dt = 1 ms with slip_velocity = 0.01 m/s chatters.
 * NMPC_E_ARG wherever a cfg is taken: cfg NULL, a field that is not finite, stiffness, damping or mu < 0, slip_velocity <= 0. */
typedef struct { float ground_z, stiffness, damping, mu, slip_velocity, tau_max; } nmpc_contact_cfg;   /* host struct, read at the call */

/* world position and velocity of every foot point: pos, vel [B][n_feet][3] (either may be NULL, not both); v NULL = zero */
int nmpc_foot_kinematics_batch(void *handle, int B, const float *q, const float *v, float *pos, float *vel, void *stream);

/* the law alone: f [B][n_feet][3], the forces nmpc_fd_accel_batch would have to be handed (v NULL = zero) */
int nmpc_contact_forces_batch(void *handle, int B, const nmpc_contact_cfg *cfg, const float *q, const float *v, float *f, void *stream);

/* nmpc_fd_step_batch with the contact forces re-evaluated from (q, v) in every substep and the torque limit applied:
 *   tau = clamp(tau_ff + kp (q_des - q_j) - kd v_j);  f = contact(q, v);  a = fd(q, v, tau, f);  v += dt a;  q += dt v
 * f_out [B][n_feet][3], tau_out [B][n_actuated]: force and clamped torque of the LAST substep (NULL allowed); q_out, v_out may
 * alias q, v.  One launch per call; f never goes through memory between substeps.  NMPC_E_ARG as nmpc_fd_step_batch and for
 * the cfg as above.  NaN rows in all outputs as nmpc_fd_accel_batch. */
int nmpc_contact_step_batch(void *handle, int B, int n_sub, float dt, const nmpc_contact_cfg *cfg, const float *q, const float *v,
                            const float *tau_ff, const float *q_des, float kp, float kd,
                            float *q_out, float *v_out, float *a_out, float *f_out, float *tau_out, void *stream);

/* A push on the contact plant [decl] (the reference pushes the MuJoCo base: data_collection_force_perturbation.py): robot b is
 * pushed with the world-frame force force[b] (N, no moment) at the origin of the body frame of joint `joint` (5: the trunk of the
 * 18-joint tree) -- in the recursion one more foot force with zero offset, so it acts inside every pushed substep, where the
 * feet and the torque limit answer it.  The attach idiom of nmpc_policy_rollout_set_states: the struct is copied at the call,
 * force (dev [force_rows][3], caller-owned, kept as a pointer) is read in stream order.  While a push is attached it acts in
 * three calls, in the substeps s with first_substep <= s < first_substep + n_substeps, s counted from 0 at the start of each call:
 *   nmpc_contact_step_batch     s = i                (substep i of the call)
 *   nmpc_contact_track_batch    s = k n_sub + i      (substep i of control step k)
 *   nmpc_policy_rollout_batch   s = k n_sub + i      (its step launches see the window moved by k n_sub; the attachment stays)
 * first_substep may be negative: the window is cut to the call's substeps, so a chain of single calls with the window moved
 * along is bit for bit the long call.  A call is cut into runs of un-pushed substeps, which are launches of the un-pushed kernels
 * (no zero force is added: their arithmetic is the one it was), and runs of pushed substeps, which are launches of one pushed
 * kernel for the step and the track alike -- up to three launches for a step, and for a track one more per control step the
 * window starts or ends in.  With nothing attached, or a window that misses the call, the launches are the ones made without.
 * nmpc_fd_step_batch, nmpc_fd_accel_batch and nmpc_contact_forces_batch are not affected.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached staying: force NULL, force_rows < 1, joint outside
 * [0, n_joints), n_substeps < 0.  At a plant call, before any launch: B > force_rows.  push = NULL detaches. */
typedef struct { const float *force; int force_rows, joint, first_substep, n_substeps; } nmpc_push_cfg;   /* host struct, copied at the call */
int nmpc_contact_set_push(void *torque, const nmpc_push_cfg *push);

/* A push window per robot [decl] (the reference pushes every perturbed rollout at a replanning point of its own for a duration of
 * its own: data_collection_pretrain_omini_vc_policy_1direction_perturbed.py:191-247).  first_substep, n_substeps: dev int [rows],
 * caller-owned, kept as pointers and read in stream order.  While they are attached they replace first_substep / n_substeps of
 * the attached nmpc_push_cfg in the three calls it acts in: robot b is pushed with force[b] in the substeps
 *   first_substep[b] <= s < first_substep[b] + n_substeps[b],
 * s counted exactly as stated there -- per call for nmpc_contact_step_batch, k n_sub + i for nmpc_contact_track_batch and
 * nmpc_policy_rollout_batch (whose step launches take k n_sub off the windows; the attachment stays), and moved by the call's
 * substep offset where a rollout makes the call.  A negative first_substep[b] is allowed, and n_substeps[b] <= 0 means no push for
 * robot b.  Robot b of such a call is bit for bit robot b of the same call (same B, same row) made without the arrays under a
 * push whose window is b's.
 * Launches: under the explicit integrator the cut into un-pushed and pushed launches is uniform over the batch and cannot serve
 * windows that differ, so a call with windows attached is ONE launch of one more kernel for the step and the track alike, in
 * which every robot takes, substep by substep, either the un-pushed substep (no force term at all) or the pushed one; under the
 * linearly implicit integrator it is the one launch it is anyway, the window test inside it reading the robot's own window.
 * With no windows attached every call makes exactly the launches it makes without this entry point.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached staying: only one of the two pointers given, rows < 1.  At a
 * plant call, before any launch: windows attached and no push attached, B > rows.  NULL, NULL detaches (the push stays). */
int nmpc_contact_set_push_windows(void *torque, const int *first_substep, const int *n_substeps, int rows);

/* A ground and a torque limit per robot [decl] (the declared law has no reference to identify its parameters from: a sweep over
 * them, and a learner that must not fit one declared floor, want them per robot).  rows: dev [n_rows][6], caller-owned, kept as a
 * pointer and read in stream order at each launch; row b is robot b's law in the field order of nmpc_contact_cfg -- ground_z,
 * stiffness, damping, mu, slip_velocity, tau_max (tau_max <= 0: no limit).  While a table is attached
 *   nmpc_contact_forces_batch, nmpc_contact_step_batch, nmpc_contact_track_batch, nmpc_policy_rollout_batch (through its step
 *   launches) and nmpc_wb_rollout_* with a plant (through its track launches)
 * read robot b's parameters from row b and ignore the values of their cfg / ground argument, which is still validated: a call
 * keeps its error behaviour.  The squared slip velocity is formed on the device as the fp32 product slip_velocity *
 * slip_velocity, the product the host forms for a cfg, so robot b of such a call is bit for bit robot b of the same call (same B,
 * same row, same push) made without a table under cfg = row b.
 * The device does NOT validate the values of a row: a caller who bypasses the Python layer owns them (what nmpc_contact_cfg is refused
 * for -- a field that is not finite, stiffness, damping or mu < 0, slip_velocity <= 0 -- gives NaN or a ground that pulls).
 * Launches: each plant call is ONE launch under either integrator, of one more instantiation of the chain kernel per integrator,
 * in which every lane keeps its law in a slot of its own behind the block's LDS slice (24 bytes per robot); an attached push --
 * none, one window, or windows per robot -- is tested per substep inside it, and under the explicit integrator every robot then
 * takes either the un-pushed substep or the pushed one, as under nmpc_contact_set_push_windows.  nmpc_contact_forces_batch
 * launches a rows-reading variant of its kernel.  With no table attached every call makes exactly the launches it makes without
 * this entry point.  nmpc_fd_step_batch and nmpc_fd_accel_batch take given forces and are not affected.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached staying: rows given and n_rows < 1.  At a call of the above,
 * before any launch: B > n_rows.  rows = NULL detaches. */
int nmpc_contact_set_grounds(void *torque, const float *rows, int n_rows);

/* A payload per robot [decl] (the other half of the randomisation a policy is trained and judged under: the robot itself).  One
 * rigid point mass per robot on one body of the tree.  rows: dev [n_rows][4], caller-owned, kept as a pointer and read in stream
 * order at each launch; row b is (m_p, r_x, r_y, r_z): robot b carries the mass m_p >= 0 at r in the frame of body `joint`.
 * While a table is attached the spatial inertia of that body about its origin is A += m_p (|r|^2 1 - r r^T), B += m_p [r]x,
 * C += m_p 1 (moment = A dw + B dvo) and its velocity-product force gains v x* (I_p v); gravity needs no term, it is the
 * acceleration of the world.  That is the tree whose body `joint` has mass m + m_p, centre of mass (m c + m_p r) / (m + m_p) and
 * the parallel-axis inertia about that point.
 * The calls that READ the table -- robot b carries row b:
 *   nmpc_contact_step_batch, nmpc_contact_track_batch, nmpc_policy_rollout_batch (through its step launches) and nmpc_wb_rollout_*
 *   with a plant (nmpc_wb_rollout_set_plant, through its track launches),
 * under the explicit and the linearly implicit integrator (whose factorised mass matrix is the payload-carrying one), with or
 * without a push, windows per robot or a table of grounds.
 * The calls that do NOT read the table -- they describe the nominal model, which is what the expert knows:
 *   nmpc_id_torques_batch, nmpc_fd_accel_batch, nmpc_fd_step_batch, nmpc_mass_matrix_batch, nmpc_centroidal_batch,
 *   nmpc_centroidal_derivatives_batch, nmpc_state_momentum_batch, nmpc_plan_actions_batch, nmpc_wb_label_states_batch, and
 *   nmpc_contact_forces_batch with nmpc_foot_kinematics_batch (kinematics only).
 * So only the plant carries the load, and the labels of the states it visits are the nominal expert's.
 * The device does NOT validate the values of a row: a caller who bypasses the Python layer owns them (a negative or non-finite
 * mass gives NaN or a body that pushes back).
 * Launches: each plant call is ONE launch under either integrator, of one more instantiation of the chain kernel per integrator,
 * in which every lane keeps its law and its payload in a slot of its own behind the block's LDS slice (40 bytes per robot); the
 * law is row b of the table of grounds if one is attached, else the call's cfg; a push is taken as under a table of grounds.
 * With no table attached every call makes exactly the launches it makes without this entry point.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached staying: rows given and n_rows < 1, or joint outside
 * [0, n_joints).  At a call of the first list, before any launch: B > n_rows.  rows = NULL detaches (n_rows, joint are not read). */
int nmpc_contact_set_payloads(void *torque, const float *rows, int n_rows, int joint);

/* An actuator per robot [decl] (the last part of the plant that the whole batch shared: a learner that outputs PD targets is
 * sensitive to the gains those targets meet before anything else, and the nominal joints have neither passive damping nor rotor
 * inertia).  rows: dev [n_rows][4], caller-owned, kept as a pointer and read in stream order at each launch; row b is
 * (kp_b, kd_b, damping_b, armature_b) -- N m/rad, N m s/rad, N m s/rad, kg m^2 -- and applies to every actuated joint of robot b.
 * While a table is attached one substep of robot b is
 *   1. the motor torque  tau_i = clamp(tau_ff_i + kp_b (q_des_i - q_i) - kd_b v_i), the clamp being the law's tau_max (row b of
 *      the table of grounds if one is attached, else the cfg); this is what tau_out reports.  kp, kd of the call are validated as
 *      they are without a table and are not read for the law;
 *   2. the joint torque handed to the dynamics  t_i = tau_i - damping_b v_i: passive, after the clamp, never cut by it;
 *   3. the dynamics of the tree whose joint-space inertia is M(q) + armature_b on the diagonal entries of the actuated joints -- in
 *      the articulated-body recursion the pivot of actuated joint i is S^T I^A S + armature_b; base joints are untouched;
 *   4. under NMPC_INTEGRATOR_LINEARLY_IMPLICIT, M is M + D_b (D_b = armature_b on the actuated diagonal) in A and in
 *      rhs = (M + D_b) a_exp - ..., and on the actuated joints the clamp did not cut  A_ii += dt (kd_b + damping_b) + dt^2 kp_b,
 *      rhs_i -= dt kp_b v_i;  on the others (cut, or no q_des)  A_ii += dt damping_b only.
 * The calls that READ the table -- robot b is driven by row b:
 *   nmpc_contact_step_batch, nmpc_contact_track_batch, nmpc_policy_rollout_batch (through its step launches) and nmpc_wb_rollout_*
 *   with a plant (nmpc_wb_rollout_set_plant, through its track launches),
 * under either integrator, with or without a push, windows per robot, a table of grounds or a table of payloads.
 * The calls that do NOT read the table -- they describe the nominal model and the nominal controller:
 *   nmpc_fd_step_batch, nmpc_fd_accel_batch, nmpc_id_torques_batch, nmpc_mass_matrix_batch, nmpc_centroidal_batch,
 *   nmpc_centroidal_derivatives_batch, nmpc_state_momentum_batch, nmpc_contact_forces_batch, nmpc_pd_torques_batch,
 *   nmpc_pd_target_action_batch, nmpc_plan_actions_batch, nmpc_wb_label_states_batch.
 * So the expert's labels (tau_id + kd v) / kp + q are formed with the nominal gains and the plant answers them with its own: the
 * torque a label produces on robot b is not the torque the expert meant.  That mismatch is the point -- it is what a learner meets
 * on a machine whose drives are not the nominal ones.
 * The device does NOT validate the values of a row: a caller who bypasses the Python layer owns them (kp_b <= 0, a negative kd_b,
 * damping_b or armature_b, or a value that is not finite gives NaN or a joint that drives itself).
 * Launches: each plant call is ONE launch under either integrator, of one more instantiation of the chain kernel per integrator,
 * in which every lane keeps its law, its payload and its actuator in a slot of its own behind the block's LDS slice (56 bytes per
 * robot); the law is taken as under a table of payloads, the payload is row b of that table or nothing where none is attached, a
 * push is taken as under a table of grounds.  With no table attached every call makes exactly the launches it makes without this
 * entry point.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached staying: rows given and n_rows < 1.  At a call of the first list,
 * before any launch: B > n_rows.  rows = NULL detaches (n_rows is not read). */
int nmpc_contact_set_actuators(void *torque, const float *rows, int n_rows);

/* An actuation delay per robot [decl] (what the batch still shared, and still had ideal: time.  A real drive chain has a transport
 * delay between a PD target being issued and the joint answering it -- bus, inference, the solve in flight; the reference
 * compensates for it, mpc.py:548-551 -- and a policy that outputs PD targets breaks on it before it breaks on friction or load).
 * delay: dev int [rows], the control steps robot b lags by.  history: dev [rows][depth][n_actuated], a shift register per robot of
 * the last `depth` issued targets, history[b][j] being the target issued j + 1 control steps before the next one.  work: dev
 * [rows][work_rows][n_actuated], scratch the applied rows of a call go to.  All three are caller-owned, kept as pointers and read
 * (history and work also written) in stream order at each launch: the library still never allocates.
 * The rule.  Feeding n_steps issued rows I[b][0 .. n_steps) gives the applied rows
 *   d = min(max(delay[b], 0), depth)                      (clamped on the device; nothing else of a row is validated)
 *   P[b][k] = k >= d ? I[b][k - d] : H[b][d - 1 - k]
 * and leaves the register holding the new last `depth` issued targets,
 *   H'[b][j] = n_steps - 1 - j >= 0 ? I[b][n_steps - 1 - j] : H[b][j - n_steps].
 * It is a pass of copies by a kernel of its own in front of the chain of control steps (one thread per robot and actuated joint);
 * no plant kernel changes, so a delayed call is bit for bit the un-delayed call on the table P.
 * While attached:
 *   nmpc_contact_track_batch (and nmpc_wb_rollout_* with a plant, through its track launches), after all refusals and before the
 *     first launch of the chain, makes ONE launch A -> work with the call's skip flags and then runs exactly as it does with
 *     A = work, a_rows = work_rows -- as one launch or cut at a push window alike.
 *   nmpc_contact_step_batch (and every step of nmpc_policy_rollout_batch) with a q_des feeds one control step, q_des -> work as
 *     dense [B][n_actuated], and runs on work; without a q_des nothing was issued and the register does not move.  The pass runs
 *     once per call, never per piece of a call cut at a push window.
 * What the records hold: A of nmpc_policy_rollout_batch, and the action rows a whole-body rollout records, are the ISSUED
 * targets -- what the controller said, not what the joint met.
 * The calls that do NOT read the table -- the nominal model and controller, and the labels: nmpc_plan_actions_batch,
 * nmpc_wb_label_states_batch, nmpc_pd_*, nmpc_fd_*, and the rest of the second list of nmpc_contact_set_actuators.  The plant alone
 * is late; the expert and its labels do not know about it, and the learner visits the states the late plant produces.
 * The unit is the control step of the call: n_sub * dt of a policy rollout or a track (10 ms at the defaults of evaluate_policy),
 * one simulation step of the expert on the plant.  A delay inside a control step would need the chain kernel to switch targets
 * mid-step; it is out of scope.
 * Because the register is the caller's and every call advances it, a chain of calls is the long call: a track of 2 K steps is bit
 * for bit two tracks of K, and a rollout in stretches (nmpc_wb_rollout_set_clock) is bit for bit the one call.  With nothing
 * attached every call makes exactly the launches it makes without this entry point; with a table of zeros every output is bit for
 * bit the un-delayed call's.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached staying: delay given and depth outside [1, NMPC_DELAY_MAX_DEPTH],
 * rows < 1, work_rows < 1, a NULL history or work.  At a plant call, before any launch: B > rows; at a track also
 * n_steps > work_rows, or A overlapping work.  delay = NULL detaches (nothing else is read). */
#define NMPC_DELAY_MAX_DEPTH 64
int nmpc_contact_set_delays(void *torque, const int *delay, float *history, int depth,
                            float *work, int work_rows, int rows);

/* The delay line alone: n_steps issued rows of B robots, robot b's row k at issued + (b * issued_rows + k) * n_actuated, through
 * the attached delay and history to applied + (b * applied_rows + k) * n_actuated by the rule above; the register moves on.
 * skip as nmpc_contact_track_batch: a skipped robot's applied rows and history are neither read nor written.  One launch,
 * stream-ordered, no allocation, no synchronisation; every output word is a copy of an input word.
 * NMPC_E_ARG before any launch: nothing attached, B > rows, n_steps < 1, issued_rows or applied_rows below n_steps, a NULL issued
 * or applied, applied overlapping issued (by the extents of the two tables from the first row of robot 0 to the last of robot
 * B - 1: tables interleaved through their row strides count as overlapping). */
int nmpc_delay_line_batch(void *torque, int B, int n_steps,
                          const float *issued, int issued_rows,
                          float *applied, int applied_rows,
                          const int *skip, int skip_mask, void *stream);

/* The integrator of the contact plant [decl].  NMPC_INTEGRATOR_EXPLICIT (the default) is the step stated above, launch for launch.
 * NMPC_INTEGRATOR_LINEARLY_IMPLICIT takes the stiff terms -- ground stiffness and damping, the friction regulariser, the PD law --
 * at the end of the substep, linearised at its start.  One substep from (q, v):
 *   1. tau = clamp(tau_ff + kp (q_des - q_j) - kd v_j)                                       (the explicit step's)
 *   2. f_k = contact(p_k, pd_k) per foot, plus the attached push in the substeps of its window;  a_exp = fd(q, v, tau, f)
 *   3. for every foot with delta_k > 0, J_k the 3 x n world Jacobian of the foot point, pd_k = J_k v:
 *        g_k = max(0, 1 - damping pd_k,z),  r_k = sqrt(|pd_k,xy|^2 + slip_velocity^2),  kz_k = stiffness g_k,
 *        C_k = blockdiag( mu f_k,z (I_2 / r_k - pd_xy pd_xy^T / r_k^3),  g_k > 0 ? stiffness delta_k damping : 0 )
 *      -- the symmetric positive semidefinite parts of -df/dpd and -df/dp; the coupling of f_xy to pd_z and p_z is dropped, so
 *      the system below is symmetric positive definite (the scheme is first-order consistent for any such choice);
 *   4. A = M(q) + sum_k (dt J_k^T C_k J_k + dt^2 kz_k J_k,z^T J_k,z),   rhs = M a_exp - dt sum_k kz_k pd_k,z J_k,z^T, and with
 *      q_des given, on every actuated joint whose torque the clamp did not cut (tau_max <= 0 or |tau_i| < tau_max):
 *      A_ii += dt kd + dt^2 kp,  rhs_i -= dt kp v_i;
 *   5. a = A^-1 rhs (L^T D L on the tree's sparsity: A couples only joints on one path to the root, as M does);
 *      v += dt a;  q += dt v.
 * a_out = a; f_out, tau_out are those of steps 1 and 2 of the last substep.  A pivot that is not a positive finite number, or an
 * unsound fd, gives the robot the NaN rows of nmpc_contact_step_batch in all outputs; other rows are untouched.
 * What it buys, on the default ground (k = 1e4, c = 3, mu = 0.8, slip_velocity = 0.05), the quadruped dropped from 2 cm, largest
 * |v| over the last 20 % of 1 s: explicit 6.7e-3 at dt = 0.5 ms, 0.46 at 1 ms (chatters), 7.0 at 2 ms; implicit below 1e-2 at
 * 0.5, 1 and 2 ms.  What it does not buy: at dt = 4 ms the implicit step no longer settles (0.78), and at slip_velocity = 0.01
 * its gain is small (0.41 at 2 ms): a factor of 4 in dt on the default ground, not more.
 * While NMPC_INTEGRATOR_LINEARLY_IMPLICIT is set, nmpc_contact_step_batch, nmpc_contact_track_batch, nmpc_policy_rollout_batch
 * (through its step launches) and nmpc_wb_rollout_* with a plant (through its track launches) run this substep, with the row
 * conventions, skip masks, in-place rules and stamps they have; each plant call is one launch of one kernel, 16 robots per
 * block, and the window of an attached push is tested per substep inside it.  A track is bit for bit the chain of its steps.
 * nmpc_fd_step_batch, nmpc_fd_accel_batch and nmpc_contact_forces_batch are never affected.
 * The slice of a robot is 54 n + n (n + 1) / 2 floats of LDS (the forward dynamics' slice and the packed triangle of A); at 16
 * robots per block a tree fits while 64 (54 n + n (n + 1) / 2) + 24 <= 163 840 bytes: n <= 35, so every tree
 * nmpc_torque_create accepts (n <= NMPC_TREE_MAX_JOINTS = 32: 144 408 bytes) fits.
 * NMPC_E_ARG (text in nmpc_torque_last_error), the previous mode staying: a mode other than the two, the implicit mode on a tree
 * beyond that bound. */
#define NMPC_INTEGRATOR_EXPLICIT 0
#define NMPC_INTEGRATOR_LINEARLY_IMPLICIT 1
int nmpc_contact_set_integrator(void *torque, int mode);

/* A policy in the loop on the contact plant [decl] (the reference: DAgger/utils/RolloutPolicy.py, PolicyController: MLP -> PD
 * target -> torque, in MuJoCo).
 *
 * The observation of a plant state: q, v [B][18] in the solver's Euler layout [x y z yaw pitch roll joints].  Every output may
 * be NULL.
 *   S       robot b's 44-slot state row (RolloutMPC.py:221) at S + b * s_stride (s_stride >= 44 floats):
 *           [phase, v_lin(3), body rates(3), joint rates(12), z, quaternion wxyz with w >= 0 (4), joints(12), base_wrt_feet(8)];
 *           phase = round(fmod(t, period) / period, 4) of the host doubles t, period; body rates and quaternion in fp64 from
 *           the fp32 state; base_wrt_feet[2f..2f+1] = q[0..1] - p_foot_f,xy with the foot points of the tree's own kinematics,
 *           the ones the contact law pushes.
 *   X       [B][44 + n_goal], the policy input: what nmpc_assemble_batch (nmpc_dataset.h) makes of that row and goal[b]
 *           ([B][n_goal], raw), bit for bit -- columns [s_first, 44) are (float)(((double)s - s_mean) / s_std), the others raw;
 *           s_mean, s_std: dev double [44], both NULL = raw.
 *   failed  dev int [B], sticky: failed[b] |= the NMPC_ROLLOUT_FLAG_* bits of nmpc.h the state raises -- roll, pitch, height,
 *           collision (z < collision_height), joint limits, and the solver bit for a height that is not finite; the velocity-
 *           tracking bit is never raised (there is no command).  If a bit of term_mask is set and failed[b] carries no stamp yet,
 *           (step_index + 1) << NMPC_ROLLOUT_TERM_SHIFT is added.
 * One launch (one more behind it, on X, while a table of nmpc_contact_set_noise is attached and X is given); with S and X NULL
 * the kinematics are not run.  NMPC_E_ARG (text in nmpc_torque_last_error): a tree that is not
 * 18 joints / 12 actuated / 4 feet, a NULL q or v, period <= 0, n_goal < 0, X without goal (n_goal > 0), only one of s_mean /
 * s_std, s_first outside [0, 44], S with s_stride < 44. */
int nmpc_observe_batch(void *handle, int B, const float *q, const float *v, double t, double period, const float *goal, int n_goal,
                       const double *s_mean, const double *s_std, int s_first, float collision_height, float *S, int s_stride,
                       float *X, int *failed, int step_index, int term_mask, void *stream);

/* n_steps control steps of observe -> policy -> contact step in one call, nothing passing through the host.  For control step
 * k = 0 .. n_steps - 1:
 *   1. nmpc_observe_batch at t = t0 + (double)(k n_sub) (double)dt: row k of S, X, flags with step index k;
 *   2. nmpc_policy_forward(policy, B, X, A_k), A_k a dense [B][12] buffer of the torque handle (the policy writes dense rows,
 *      and row k of A is strided), copied into row k of A when A is given; the handle allocates the buffer the first time a
 *      batch larger than any before needs it -- the one allocation of this header, and none in any later call.  That call
 *      frees and allocates, which synchronises the device and cannot be captured into a graph; every other call synchronises
 *      nothing.  The buffer belongs to the handle: one rollout per torque handle at a time, whatever the streams;
 *   3. nmpc_contact_step_batch with q_des = A_k (actions are PD targets in joint order, as the labels are), n_sub substeps in
 *      place on q, v;
 * then one more observation with S and X NULL and step index n_steps, so that a robot that falls in the last interval is seen.
 * S, A, q, v and failed are bit for bit those of that chain of the three public calls.
 * No freeze: robots are independent, a NaN row stays in its row, a terminated robot keeps being stepped and its later rows
 * are written as the plant produces them; the stamp in failed[b] (1 + the control step whose observation terminated it) tells
 * the consumer where to cut.  Stream-ordered; no synchronisation but for the growth of the action buffer above.
 * NMPC_E_ARG (text in nmpc_torque_last_error): a NULL torque, policy, cfg, ground, q, v, goal or X; n_steps < 1, n_sub < 1,
 * dt <= 0, period <= 0; kp not finite; only one of s_mean / s_std; s_first outside [0, 44]; n_goal < 0; a policy whose
 * n_in != 44 + n_goal or n_out != 12; B > its batch_max; a policy on another device; a tree that is not 18 / 12 / 4; a ground
 * cfg nmpc_contact_step_batch refuses.  A failing nmpc_policy_forward returns its code, its text copied over. */
typedef struct { int n_steps, n_sub; float dt, kp, kd; double t0, period; float collision_height; int term_mask, n_goal, s_first; } nmpc_policy_rollout_cfg;
int nmpc_policy_rollout_batch(void *torque, void *policy, int B, const nmpc_policy_rollout_cfg *cfg, const nmpc_contact_cfg *ground,
                              float *q, float *v,                 /* [B][18] in: start state, out: final state */
                              const float *tau_ff,                /* [B][12] constant feed-forward or NULL */
                              const float *goal,                  /* [B][n_goal] */
                              const double *s_mean, const double *s_std,   /* dev [44] or both NULL */
                              float *S, float *A,                 /* [B][n_steps][44], [B][n_steps][12]; either may be NULL */
                              float *X,                           /* workspace [B][44 + n_goal] */
                              int *failed,                        /* dev [B], sticky, caller zeroes; NULL allowed */
                              void *stream);

/* The plant states beside a policy rollout: the attach idiom of nmpc_wb_rollout_set_actions (nmpc.h).  While Q, V (dev, caller-
 * owned, kept as pointers) are attached, every nmpc_policy_rollout_batch of this handle writes the plant state BEFORE control
 * step k to Q + (b * qv_rows + k) * 18, and V alike -- nmpc_contact_track_batch's row convention, so row k goes with row k of S
 * and A; these are the states a solver can start from (the 44-slot rows drop x, y and the Euler layout).  One strided-copy launch
 * per control step; every other output of the rollout is bit for bit what it is without.  Q = V = NULL detaches; detached, the
 * launches of a rollout are exactly what they are without this call, and nmpc_policy_rollout_cfg is unchanged.  A rollout with
 * only one of Q / V attached, or with qv_rows < n_steps, returns NMPC_E_ARG before any launch. */
int nmpc_policy_rollout_set_states(void *torque, float *Q, float *V, int qv_rows);

/* Sensor noise and bias per robot on the policy input [decl] (the push, the ground, the payload, the actuator and the delay are
 * all on the output side of the learner; its input was still ideal: the policy read the plant state to the last bit.  A policy
 * that outputs PD targets from joint encoders, an IMU and a state estimator never does, and noise is what drives a DAgger
 * learner into the states the expert is there to label).
 * noise: dev float [rows][88], caller-owned and kept as a pointer, read in stream order at each launch: row b holds sigma[44] and
 * then bias[44], in the units of the RAW 44-slot row.  seed: the 64 bits of the key.  first_robot: robot b of a call draws as
 * robot first_robot + b of the population, so that shards of one population draw distinct streams.  step0: the handle's noise
 * step from now on.
 * The rule.  For robot b, r = first_robot + b taken mod 2^32, noise step s taken mod 2^32, slot j, 0 <= j < 44:
 *   (w0, w1) = the first two words of Philox-4x32-10 with counter (r, s, j, 0) and key (seed lo, seed hi)
 *   t = (w0 & 0xffff) + (w0 >> 16) + (w1 & 0xffff) + (w1 >> 16) - 131070                   an integer, |t| <= 131070
 *   g = (float)t * c,  c = (float)(1 / sqrt((2^32 - 1) / 3))                               one fp32 product
 *   n = (double)bias[j] + (double)sigma[j] * (double)g                                     each operation rounded once, no fma
 *   X[b][j] <- (float)((double)X[b][j] + n / s_std[j])     where s_std is given and j >= s_first (the normalised columns)
 *   X[b][j] <- (float)((double)X[b][j] + n)                elsewhere
 * g is the centred sum of four uniforms on 0 .. 65535 scaled to unit variance: zero mean, |g| < 3.4641, no transcendental, so a
 * restatement on the host gives the same bits.  A slot with sigma[j] == 0 and bias[j] == 0 is not written; the goal columns
 * behind slot 43 are never touched.  A kernel of its own, one thread per (robot, slot); nothing else of the table is validated on
 * the device.
 * While attached, every nmpc_observe_batch that is given an X makes ONE more launch behind its own -- the rule on that X with
 * x_stride = 44 + n_goal and the call's s_std, s_first, at the handle's noise step -- and then advances the step by one.  An
 * observation without an X, such as the last one of a rollout, draws nothing and advances nothing.  nmpc_policy_rollout_batch
 * inherits this through its observations and stays bit for bit the chain of the public calls; because the step moves on, two
 * rollouts of K control steps are the rollout of 2 K.
 * What does not change: S, failed, the rows Q, V of nmpc_policy_rollout_set_states, the plant, the delay register and every label
 * are the bits they are without a table -- only what the policy is shown moves, and through its actions the states visited.
 * With nothing attached every call makes exactly the launches it makes without this entry point.
 * The step is host state of the handle: a captured graph replays the one step value it was captured with.  Capture is out of
 * scope here.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached and its step staying: rows < 1.  At nmpc_observe_batch with an X
 * and at nmpc_policy_rollout_batch, before any launch: B > rows.  noise = NULL detaches (nothing else is read). */
int nmpc_contact_set_noise(void *torque, const float *noise, int rows, long long seed, long long first_robot, long long step0);

/* The noise step the next observation with an X draws at.  NMPC_E_ARG: a NULL step, nothing attached. */
int nmpc_contact_noise_step(void *torque, long long *step);

/* The rule alone, on the B rows of X (robot b's at X + b * x_stride, x_stride >= 44; its first 44 slots are read and written), at
 * the given step: the handle's noise step is neither read nor moved.  s_std: dev double [44] or NULL (X is raw); s_first as
 * nmpc_observe_batch.  For the chain of the public calls, and for a caller who perturbs a training batch.  One launch,
 * stream-ordered, no allocation, no synchronisation.
 * NMPC_E_ARG before any launch: nothing attached, B > rows, a NULL X, x_stride < 44, s_first outside [0, 44]. */
int nmpc_observe_noise_batch(void *torque, int B, float *X, int x_stride, const double *s_std, int s_first, long long step,
                             void *stream);

/* The rows the sensors showed [decl]: the raw 44-slot row in the units of the database's state table, as robot b's sensors show
 * it at noise step `step` -- the handle's own noise step is neither read nor moved.  For robot b (its true row at S + b *
 * s_stride, its observed row at O + b * o_stride) and slot j < 44, with n exactly the n of nmpc_contact_set_noise's rule at counter
 * (first_robot + b, step, j, 0), the draw that perturbs X at that step:
 *   O[b][j] = (float)((double)S[b][j] + n)     where sigma[j] != 0 || bias[j] != 0
 *   O[b][j] = S[b][j], the same bits           elsewhere, and whenever no table is attached
 * Where X is raw, the first 44 columns of the perturbed X of that step are this row to the bit; where X is normalised the two
 * differ by roundings.  O may be S: every element is read and written by its own thread alone.  A kernel of its own, one thread
 * per (robot, slot): one launch, stream-ordered, no allocation, no synchronisation.
 * NMPC_E_ARG before any launch: a NULL S or O, a stride below 44, B > rows while a table is attached. */
int nmpc_observed_rows_batch(void *torque, int B, const float *S, int s_stride, float *O, int o_stride, long long step, void *stream);

/* The observed rows beside a policy rollout, attached as nmpc_policy_rollout_set_states attaches Q, V: O is dev float
 * [B][o_rows][44], caller-owned and kept as a pointer.  While attached, control step k of every nmpc_policy_rollout_batch of the
 * handle writes robot b's observed row to O + (b * o_rows + k) * 44 by ONE more launch per control step:
 * nmpc_observed_rows_batch on the step's true row at the noise step the step's observation drew X at -- read before the
 * observation advances it, so row k of O and the input the policy acted on in step k are one draw.  With a rollout whose S is
 * NULL the observation writes the true row into O's row and the launch perturbs it in place.  O is bit for bit the chain
 * nmpc_contact_noise_step, nmpc_observe_batch, nmpc_observed_rows_batch at the step read; with no table of noise attached it is
 * S.  S, A, q, v, failed, the Q, V of nmpc_policy_rollout_set_states, the delay register and the noise step are the bits they
 * are without O.  O = NULL detaches.  A rollout with o_rows < n_steps returns NMPC_E_ARG before any launch. */
int nmpc_policy_rollout_set_observed(void *torque, float *O, int o_rows);

/* Observation and action history on the policy input [decl] (a robot's ground, payload, actuator, delay and sensor bias do not
 * stand in one 44-slot row: they show in how successive rows and the issued PD targets relate, so a memoryless policy cannot
 * identify them).  With n_obs >= 1 observed rows and n_act >= 0 previous actions, n_wide = 44 n_obs + 12 n_act, and the raw wide
 * row of robot b in control step k is
 *   W_k = [ O_k | O_{k-1} | ... | O_{k-n_obs+1} | A_{k-1} | ... | A_{k-n_act} ]
 * O_j the raw 44-slot row as the robot's sensors showed it in step j (nmpc_observed_rows_batch of the true row at that step's
 * noise step; S_j to the bit without a table of noise), A_j the PD target ISSUED in step j (what A records, not what a delayed
 * joint met).  Before step 0 an entry is whatever the register held.  The policy input is X_k = [normalise(W_k), goal]: column c
 * in [s_first, n_wide) is (float)(((double)w - s_mean[c]) / s_std[c]), the others are raw, the goal follows raw -- the expression
 * of nmpc_assemble_batch on a table of n_state = n_wide, so what a database makes of a stored wide row is bit for bit what the
 * policy was shown.  With a table of noise X_k[:44] is normalise(O_k), the quotient taken once on the perturbed row; that differs
 * by roundings from the memoryless input normalise(S) + n / s_std of nmpc_contact_set_noise.  With a history attached deployment
 * and training see identical inputs.
 * Two registers, both dev float, caller-owned and kept as pointers; the library still never allocates:
 *   hist [rows][n_obs][44]   slot 0 is the incoming slot: the caller or the rollout writes step k's observed row there (for
 *                            example nmpc_observed_rows_batch with o_stride = 44 n_obs); slot h is the row of h steps ago
 *   act  [rows][n_act][12]   slot i is the target issued i + 1 steps before the next one, the delay register's convention
 * NMPC_HISTORY_MAX bounds both depths. */
#define NMPC_HISTORY_MAX 16

/* The wide row of B robots out of their registers, then the observed rows age.  One launch, one thread per (robot, column of
 * 44 + 12 + n_goal).  Thread (b, j < 44) reads column j of all n_obs slots of robot b, writes the n_obs entries of W (robot b's
 * row at W + b * w_stride, w_stride >= n_wide; the words behind n_wide are not touched) and of X ([B][n_wide + n_goal], dense)
 * that are made of them, and ages its column in place, slot h + 1 <- slot h from the oldest down; slot 0 keeps its content.
 * Thread (b, 44 + i) writes the n_act entries of joint i and moves nothing (nmpc_history_push_actions_batch moves them); the goal
 * threads copy the goal [B][n_goal] behind the wide row of X.  Either of W and X may be NULL, not both.  s_mean, s_std: dev double
 * [n_wide] or both NULL (X is raw); the quotient is taken in fp64 as nmpc_assemble_batch takes it.  Every word of W is a copy of an
 * input word; no thread reads a word another thread writes, provided W and X overlap neither register.  Stream-ordered, no
 * allocation, no synchronisation.
 * NMPC_E_ARG before any launch (text in nmpc_torque_last_error): a NULL hist, a NULL act with n_act > 0, W and X both NULL; B < 1;
 * n_obs outside [1, 16], n_act outside [0, 16]; w_stride < n_wide with a W; only one of s_mean / s_std; s_first outside
 * [0, n_wide]; n_goal < 0; an X with n_goal > 0 and no goal; a tree that is not 18 / 12 / 4. */
int nmpc_history_push_batch(void *torque, int B, float *hist, int n_obs, const float *act, int n_act, const float *goal, int n_goal,
                            const double *s_mean, const double *s_std, int s_first, float *W, int w_stride, float *X, void *stream);

/* The action register of B robots moves on by one control step: slot s <- slot s - 1 from the oldest down, then slot 0 <- the
 * target just issued, robot b's at A + b * a_stride (a_stride >= 12).  One launch, one thread per (robot, joint); every word is a
 * copy.  NMPC_E_ARG before any launch: a NULL act or A; B < 1; n_act outside [1, 16]; a_stride < 12; a tree that is not 18 / 12 / 4. */
int nmpc_history_push_actions_batch(void *torque, int B, float *act, int n_act, const float *A, int a_stride, void *stream);

/* The history on the policy input of a policy rollout, attached as nmpc_policy_rollout_set_observed attaches O.  While hist
 * [rows][n_obs][44] and act [rows][n_act][12] are attached, nmpc_policy_rollout_batch takes a policy of n_wide + n_goal inputs, a
 * workspace X [B][n_wide + n_goal] and statistics s_mean, s_std [n_wide], and its control step k is bit for bit this chain of the
 * public calls:
 *   1. nmpc_contact_noise_step (with a table of noise attached);
 *   2. nmpc_observe_batch exactly as without a history: its narrow X [B][44 + n_goal] goes into the head of the workspace, with a
 *      table of noise it draws and the noise step moves on by one;
 *   3. nmpc_observed_rows_batch of the step's true row into slot 0 of hist (o_stride = 44 n_obs) at the step read -- in addition
 *      to the launch into an attached O; in a rollout with neither S nor O the observation writes the true row into slot 0 and it is
 *      perturbed in place;
 *   4. nmpc_history_push_batch into row k of W (robot b's at W + (b * w_rows + k) * n_wide) if W is given, and into the workspace
 *      X, overwriting it;
 *   5. nmpc_policy_forward;
 *   6. the contact step as without a history, the delay line included;
 *   7. nmpc_history_push_actions_batch of the issued dense actions, if n_act > 0.
 * Two or three more launches per control step.  S, failed, the Q, V of nmpc_policy_rollout_set_states, the delay register, O and
 * the noise step are the bits they are without a history when the policy is fed the same input; at (n_obs, n_act) = (1, 0) without
 * noise the rollout is the one without a history and W is S.  Both registers move with every step, so two rollouts of K control
 * steps are the rollout of 2 K; the caller fills them before the first (a posture and its row, say).  W: dev float
 * [rows][w_rows][n_wide] or NULL.  hist = NULL detaches (nothing else is read); detached, every call makes exactly the launches
 * it makes without this entry point.  Capture into a graph is out of scope, as for the noise step.
 * NMPC_E_ARG (text in nmpc_torque_last_error), what was attached staying: n_obs outside [1, 16]; n_act outside [0, 16]; a NULL act
 * with n_act > 0; rows < 1; w_rows < 1 with a W.  At nmpc_policy_rollout_batch, before any launch: B > rows; w_rows < n_steps; a
 * policy whose n_in != n_wide + n_goal. */
int nmpc_policy_rollout_set_history(void *torque, float *hist, int n_obs, float *act, int n_act, float *W, int w_rows, int rows);

/* A table of PD targets tracked on the contact plant [decl]: n_steps control steps in one launch, control step k being n_sub
 * substeps of nmpc_contact_step_batch's law with q_des = row k of robot b's table, at A + (b * a_rows + k) * 12 (a_rows >=
 * n_steps; 12 = n_actuated).  With the label rows of nmpc_plan_actions_batch as the table, A = (tau_id + kd v_plan) / kp + q_plan,
 * the PD law is tau = kp (A - q) - kd v = tau_id + kp (q_plan - q) + kd (v_plan - v): the reference's _compute_pd_torques
 * (mpc.py:592-599) on the plan's inverse-dynamics torque -- the whole-body expert driving the plant for a replanning interval.
 * q, v [B][n_joints] are in/out; tau_ff [B][12] is a constant feed-forward torque or NULL; Q, V (both or neither) take the state
 * BEFORE control step k at + (b * qv_rows + k) * 18 (qv_rows >= n_steps), so row 0 is the start state and row k goes with
 * row k of A.  skip: dev int [B] or NULL; a robot with skip[b] & skip_mask != 0 is left out entirely (its q, v and its rows of
 * Q, V stay as they are; read in stream order).  The state stays in the LDS over all n_steps * n_sub substeps; per control step
 * the 12 targets come in and, if asked for, 36 floats of state go out.
 * q, v, Q, V are bit for bit those of the chain of n_steps calls nmpc_contact_step_batch(.., q, v, tau_ff, A[:, k], kp, kd,
 * q, v, NULL, NULL, NULL), NaN rows of a massless leaf included: the NaN is first written where the chain first writes it.
 * NMPC_E_ARG (text in nmpc_torque_last_error) as nmpc_contact_step_batch, and: n_steps < 1, A NULL, a_rows < n_steps, only one
 * of Q / V, qv_rows < n_steps, a tree that is not 18 / 12 / 4 when Q is given. */
int nmpc_contact_track_batch(void *handle, int B, int n_steps, int n_sub, float dt, const nmpc_contact_cfg *cfg, float *q, float *v,
                             const float *tau_ff, const float *A, int a_rows, float kp, float kd, float *Q, float *V, int qv_rows,
                             const int *skip, int skip_mask, void *stream);

/* nmpc_observe_batch for the rows k = 0 .. n_rows - 1 of every robot's table of states, in one launch: row k of Q, V (at
 * + (b * qv_rows + k) * 18) observed at t = t0 + (double)k * dt_row (the product and the sum each rounded once, as a host
 * computes them) goes to S + (b * s_rows + k) * 44 (S may be NULL: flags only); failed[b] |= the bits of all rows, and after the
 * rows the stamp (step_index + 1) << NMPC_ROLLOUT_TERM_SHIFT under nmpc_observe_batch's rule (a bit of term_mask is set and no
 * stamp is present).  One thread per robot runs over its rows, so the result does not depend on scheduling.  skip as
 * nmpc_contact_track_batch: a skipped robot's rows and flags are untouched.
 * S and failed are bit for bit those of n_rows calls nmpc_observe_batch(.., Q[:, k], V[:, k], t0 + k dt_row, period, NULL, 0,
 * NULL, NULL, 0, collision_height, S + 44 k, 44 s_rows, NULL, failed, step_index, term_mask, ..).
 * NMPC_E_ARG: a tree that is not 18 / 12 / 4, a NULL Q or V, period <= 0, n_rows < 1, qv_rows < n_rows, S with s_rows < n_rows. */
int nmpc_observe_rows_batch(void *handle, int B, int n_rows, const float *Q, const float *V, int qv_rows, double t0, double dt_row,
                            double period, float collision_height, float *S, int s_rows, int *failed, int step_index, int term_mask,
                            const int *skip, int skip_mask, void *stream);

/* _compute_pd_torques: tau_ff [B][nu] (NULL = 0); q, v, q_plan, v_plan [B][n_joints] (their last nu
 * entries are used); tau [B][nu] (may alias tau_ff). */
int nmpc_pd_torques_batch(void *handle, int B, const float *tau_ff, const float *q, const float *v,
                          const float *q_plan, const float *v_plan, float kp, float kd, float *tau,
                          void *stream);

/* Recorded action: action[b][i] = (tau[b][perm[i]] + kd v[b][nj - nu + i]) / kp + q[b][nj - nu + i].
 * perm [nu] (device, NULL = identity) maps the actuator order of tau to the joint order (the
 * reference's ctrl is [FR, FL, RR, RL], its joints [FL, FR, RL, RR]: RolloutMPC.py:229-235). */
int nmpc_pd_target_action_batch(void *handle, int B, const float *tau, const int *perm, const float *q,
                                const float *v, float kp, float kd, float *action, void *stream);

/* The action labels of one plan of the whole-body model: for rollout b and step j (0 <= j < n_steps) the recorded action
 * (RolloutMPC.py:228-250) of the expert's torque at simulation step j of the interval that follows the replan,
 *     A[b][j][i] = (tau[perm[i]] + kd v[6 + i]) / kp + q[6 + i],   tau = id_torques(q, v, a, f)          (mpc.py:583)
 *   q, v   the plan at t = (j + 1) sim_dt on the cubic Hermite segments of interpolate_trajectory_with_derivatives
 *          (mpc.py:388-414; fp64 from the fp32 plan, velocities through (v_k, a_max(k-1,0))) -- the expressions, in one
 *          shared device function, with which the device rollouts record state row j, so a label sits on the state of its row;
 *   a, f   U[b][zoh[j]]: accelerations U[..][0..18), world-frame foot forces U[..][18..30) as [foot][3] -- the zero-order hold
 *          a_plan = a_sol[id_repeat], f_plan = f_sol[id_repeat] (mpc.py:142), indexed with the same j as the state, as
 *          mpc.py:583 does with plan_step.  zoh: dev int [n_steps], filled by the host from id_repeat (entries are clamped to [0, N)).
 * The plant follows the plan, so the reference's PD term Kp (q_plan - q) + Kd (v_plan - v) (mpc.py:592-599) is zero [decl] and
 * tau is the inverse-dynamics torque alone; it comes out in joint order [FL, FR, RL, RR], so perm (dev [12], as
 * nmpc_pd_target_action_batch) is NULL unless the caller wants another order.
 * X [B][N+1][42], U [B][N][30]: trajectories of NMPC_MODEL_WHOLEBODY with node spacing dt_nodes; skip: dev int [B] or NULL, a
 * rollout with skip[b] & skip_mask != 0 is left out (its rows of A stay as they are, it costs no time; read in stream order);
 * A: dev, rollout b's rows start at A + b * a_rows * 12 and the first n_steps of them are written (a_rows >= n_steps; a
 * dense [B][n_steps][12] has a_rows = n_steps).  One thread per (rollout, step).
 * NMPC_E_ARG (text in nmpc_torque_last_error): a tree that is not 18 joints / 12 actuated / 4 feet, n_steps < 1, zoh NULL,
 * kp = 0, n_steps sim_dt beyond the horizon. */
int nmpc_plan_actions_batch(void *handle, int B, int n_steps, int N, const float *X, const float *U, const int *zoh,
                            double dt_nodes, double sim_dt, float kp, float kd, const int *perm, const int *skip,
                            int skip_mask, float *A, int a_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
