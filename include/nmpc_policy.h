/* nmpc_policy.h -- C-ABI of the learning update: the reference's policy network
 * and its behaviour-cloning training step as hand-written gfx950 kernels (libnmpc_hip.so).
 *
 * Replaces, for batches that already live on the device (rollout states from nmpc_rollout_batch,
 * expert actions from nmpc_solve_batch):
 *   GoalConditionedPolicyNet.forward              DAgger/utils/network.py:72-81
 *       in -> [Linear, BatchNorm1d, ReLU] x L -> Linear -> out
 *   one iteration of BehavioralCloning.train_network   DAgger/utils/train_locosafedagger.py:93-102
 *       optimizer.zero_grad(); loss = L1Loss(network(x), y); loss.backward(); optimizer.step()   (Adam)
 * All tensors are fp32 device pointers, row-major [batch][feature]; calls are stream-ordered, never
 * allocate and never synchronise.  Return values: NMPC_OK / NMPC_E_* of nmpc.h.
 *
 * Parameter vector theta (the order of torch's net.parameters()): for each hidden layer
 * W[hidden][fan_in], b[hidden], then gamma[hidden], beta[hidden] if batch_norm; finally
 * W[n_out][hidden], b[n_out].  BatchNorm buffers: running_mean[L][hidden], running_var[L][hidden]. */
#ifndef NMPC_POLICY_H
#define NMPC_POLICY_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int n_in;        /* policy input: state + goal (47 in cfgs/iter_locosafedagger.yaml)      */
    int n_out;       /* action dimension (12)                                                 */
    int n_hidden;    /* hidden layers L >= 1 (3)                                              */
    int hidden;      /* nodes per hidden layer (512)                                          */
    int batch_norm;  /* BatchNorm1d between Linear and ReLU (1)                               */
    int batch_max;   /* largest batch of a forward / training call                            */
} nmpc_policy_dims;

int nmpc_policy_create(const nmpc_policy_dims *dims, int device_id, void **handle);
void nmpc_policy_destroy(void *handle);
const char *nmpc_policy_last_error(void *handle);

/* length of theta */
size_t nmpc_policy_param_count(void *handle);

/* the dims the handle was created with and the device it lives on (either pointer may be NULL) */
int nmpc_policy_get_dims(void *handle, nmpc_policy_dims *dims, int *device_id);

/* Copy parameters and BatchNorm buffers in / out (device pointers; running_* may be NULL without
 * batch_norm).  set_params also resets the optimiser state (Adam moments, step count). */
int nmpc_policy_set_params(void *handle, const float *theta, const float *running_mean,
                           const float *running_var, void *stream);
int nmpc_policy_get_params(void *handle, float *theta, float *running_mean, float *running_var,
                           void *stream);

/* The optimiser state, for checkpoint / resume and for tests that need the gradient: Adam's first and second moments
 * m, v (device pointers, param_count floats each, in the layout of theta) and the count of steps taken (it sets the
 * bias corrections 1 - beta^step of the next step).  The copies are device to device and asynchronous on the stream.
 *   get: any of m, v, step may be NULL; step is host state and is written at once -- it counts the steps launched so
 *        far, whose moments the copies deliver in stream order.
 *   set: needs m, v and step >= 0 (NMPC_E_ARG otherwise, nothing changed); step 0 with zero moments is the state
 *        set_params leaves.  To resume a run, call set_params first (it resets the state), then this.
 * After one step from the reset state m = (1 - 0.9f) g, so the gradient g of that step can be read off m. */
int nmpc_policy_get_opt_state(void *handle, float *m, float *v, long long *step, void *stream);
int nmpc_policy_set_opt_state(void *handle, const float *m, const float *v, long long step, void *stream);

/* network.eval(); Y = network(X)      X[B][n_in] -> Y[B][n_out] */
int nmpc_policy_forward(void *handle, int B, const float *X, float *Y, void *stream);

/* One Adam step on the L1 loss of a batch (train mode: batch statistics, running statistics updated
 * with momentum 0.1).  loss: device scalar, the mean absolute error BEFORE the step (may be NULL);
 * pred: the train-mode prediction [B][n_out] (may be NULL).  B >= 2 with batch_norm. */
int nmpc_policy_train_step(void *handle, int B, const float *X, const float *Y, float lr, float *loss,
                           float *pred, void *stream);

/* torch.utils.data.WeightedRandomSampler(weights, num_samples, replacement=True)
 * (Behavior_Cloning/examples/test_train_policy.py:128-134) on device weights -- e.g. the OOD weights
 * nmpc_tracking_error wrote:  idx[i] ~ weights / sum(weights),  0 <= i < num_samples.  Sample i is the
 * inverse-CDF lookup of a uniform number made by the counter-based Philox-4x32-10 generator from
 * (seed, i): reproducible for a seed whatever the launch shape, and restated bit for bit by the oracle.
 * scratch: n + n/2048 + 2 doubles of device memory.  Stateless (no handle). */
int nmpc_weighted_sample(const float *weights, long long n, int num_samples, unsigned long long seed,
                         double *scratch, int *idx, void *stream);

/* Batch assembly behind the sampler: dst[i][0..row_len) = src[idx[i]][0..row_len) for a table of n_rows
 * rows; an idx outside [0, n_rows) is not read, its output row is NaN. */
int nmpc_gather_rows(const float *src, long long n_rows, int row_len, const int *idx, int n_idx, float *dst,
                     void *stream);

/* The tables a batch is assembled from: the arguments of nmpc_assemble_batch (nmpc_dataset.h), with the same
 * meaning -- s_mean/s_std NULL: states raw; states normalised from column s_first on; g_mean/g_std NULL: goals raw;
 * n_rows: rows of the three tables. */
typedef struct {
    const float *states;  int n_state;  const double *s_mean, *s_std;  int s_first;
    const float *goals;   int n_goal;   const double *g_mean, *g_std;
    const float *actions; int n_action;
    long long n_rows;
} nmpc_batch_source;

/* One epoch of BehavioralCloning.train_network (DAgger/utils/train_locosafedagger.py:93-102) in one call: n_batches
 * Adam steps on batches of `batch` rows drawn from src with replacement, row r with probability
 * weights[r] / sum(weights) (weights: n_rows floats).  Step t trains on rows idx[t*batch + j], j < batch, where idx
 * is the sequence nmpc_weighted_sample gives for (weights, n_rows, n_batches*batch, seed), assembled as
 * nmpc_assemble_batch assembles them and stepped as nmpc_policy_train_step steps: parameters, running statistics,
 * optimiser state and losses are bit for bit those of that chain of calls.  The prefix sums of the weights are made
 * once per call; a row of weight zero is never drawn.  All-zero or non-finite weights have the behaviour they have
 * in nmpc_weighted_sample: no guarantee.
 *   scratch: nmpc_policy_train_epoch_scratch of n_rows doubles (the prefix sums and their block totals: the size
 *            rule of nmpc_weighted_sample)
 *   losses:  n_batches floats, the loss BEFORE each step
 *   idx_out: n_batches*batch ints, the rows drawn, or NULL
 * Needs src->n_state + src->n_goal == n_in, src->n_action == n_out, 1 <= batch <= batch_max (2 <= batch with
 * batch_norm), n_batches >= 0 (0: nothing happens), n_batches*batch < 2^31, 1 <= n_rows < 2^31, lr > 0. */
size_t nmpc_policy_train_epoch_scratch(long long n_rows);
int nmpc_policy_train_epoch(void *handle, const nmpc_batch_source *src, const float *weights, int batch,
                            int n_batches, unsigned long long seed, float lr, double *scratch, float *losses,
                            int *idx_out, void *stream);

/* Input noise on the batches of nmpc_policy_train_epoch [decl]: a policy that is deployed behind noisy sensors
 * (nmpc_contact_set_noise, nmpc_torque.h) is trained on perturbed inputs, and the epoch call assembles its batches inside the
 * library, so the perturbation is attached to the handle.
 * sigma: dev float [n], caller-owned and kept as a pointer, read in stream order at each launch, in the units of the RAW input
 * columns 0 .. n-1, 1 <= n <= n_in.  seed: the 64 bits of the key.  epoch0: the handle's noise epoch from now on.
 * The rule.  For row i of a call and column j < n:
 *   (w0, w1) = the first two words of Philox-4x32-10 with counter ((first_sample + i) mod 2^32, epoch mod 2^32, j, 1) and key
 *              (seed lo, seed hi)
 *   t, g as in the sensor rule of nmpc_contact_set_noise: t the centred sum of the four 16-bit halves, g = (float)t * c
 *   nz = (double)sigma[j] * (double)g
 *   X[i][j] <- (float)((double)X[i][j] + nz / s_std[j])     where s_std is given and j >= s_first (the normalised columns)
 *   X[i][j] <- (float)((double)X[i][j] + nz)                elsewhere
 * each operation rounded once, no fma.  A column with sigma[j] == 0 is not written; columns from n on are never addressed.  The
 * fourth counter word 1 keeps these streams apart from the sensor noise of a rollout (word 0) under a shared seed.  A kernel of
 * its own, one thread per (row, column); nothing of sigma is validated on the device.
 * While attached, nmpc_policy_train_epoch makes ONE more launch per batch, between the assembly of the batch and its step, on the
 * staged x: the rule with first_sample = t * batch for batch t, at the handle's epoch, with s_std and s_first of the call's
 * nmpc_batch_source.  It needs n <= src->n_state (NMPC_E_ARG before any launch otherwise).  A call with n_batches > 0 then
 * advances the handle's epoch by one; n_batches == 0 advances nothing.  The epoch is bit for bit the chain: the idx of the epoch,
 * nmpc_assemble_batch of idx[t], nmpc_policy_input_noise_batch(epoch, first_sample = t * batch), nmpc_policy_train_step.
 * nmpc_policy_train_step, nmpc_policy_forward and nmpc_policy_loss never draw: validation stays on clean rows.  With nothing
 * attached every call makes exactly the launches it makes without this entry point.  The epoch is host state of the handle;
 * graph capture is out of scope.
 * NMPC_E_ARG, what was attached and its epoch staying: n outside [1, n_in].  sigma = NULL detaches (nothing else is read). */
int nmpc_policy_set_input_noise(void *policy, const float *sigma, int n, long long seed, long long epoch0);

/* The epoch the next nmpc_policy_train_epoch draws at.  NMPC_E_ARG: a NULL epoch, nothing attached. */
int nmpc_policy_input_noise_epoch(void *policy, long long *epoch);

/* The rule alone, on the B rows of X (row i at X + i * x_stride; its first n columns are read and written), at the given epoch
 * and first sample: the handle's epoch is neither read nor moved.  s_std: dev double [>= n] or NULL (X is raw).  One launch,
 * stream-ordered, no allocation, no synchronisation.
 * NMPC_E_ARG before any launch: nothing attached, a NULL X, x_stride < n, s_first < 0. */
int nmpc_policy_input_noise_batch(void *policy, int B, float *X, int x_stride, const double *s_std, int s_first,
                                  long long epoch, long long first_sample, void *stream);

/* network.eval(); mean |network(X) - Y| over n rows, n of any size >= 1 (the validation loss of
 * train_locosafedagger.py:129-132).  X[n][n_in], Y[n][n_out], loss: device scalar.  Parameters, running statistics
 * and optimiser state are not touched.  The sum runs in a fixed order, in float64 across blocks: the same bits on
 * every run. */
int nmpc_policy_loss(void *handle, long long n, const float *X, const float *Y, float *loss, void *stream);

#ifdef __cplusplus
}
#endif
#endif
