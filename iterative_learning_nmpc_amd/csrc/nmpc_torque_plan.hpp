// nmpc_torque_plan.hpp -- what the rollout host code (nmpc_api.hip) asks of the torque layer (nmpc_torque.hip) beyond its
// C-ABI: whether a label launch, or the launches of an attached plant, would be refused with these arguments, so that a rollout
// refuses before it launches anything.
#pragma once

#include "../../include/nmpc_torque.h"

namespace nmpc_torque {

// nullptr if nmpc_plan_actions_batch accepts (handle, n_steps, zoh, kp) and the handle lives on `device` (-1: any device);
// otherwise the text nmpc_torque_last_error would give
const char* plan_actions_refusal(void* handle, int n_steps, const int* zoh, float kp, int device);

// nullptr if nmpc_wb_label_states_batch (include/nmpc.h) can label n_rows states per robot with this handle: the one-step
// nmpc_plan_actions_batch of every plan is accepted (handle, zoh, kp, device as above) and the tables have their rows
// (qv_rows >= n_rows, a_rows >= n_rows, n_rows >= 1); otherwise the text nmpc_last_error gives
const char* label_states_refusal(void* handle, int n_rows, int qv_rows, int a_rows, const int* zoh, float kp, int device);

// nullptr if nmpc_contact_track_batch with rows Q, V and nmpc_observe_rows_batch accept (handle, ground, n_sub, dt) and the handle
// lives on `device` (-1: any device); otherwise the text nmpc_torque_last_error would give
const char* contact_track_refusal(void* handle, const nmpc_contact_cfg* ground, int n_sub, float dt, int device);

// has the caller attached a push to the handle (nmpc_contact_set_push)
bool push_attached(void* handle);

// a push window per robot (nmpc_contact_set_push_windows): dev int [rows] each, first == nullptr: none
struct PushWindows {
    const int *first = nullptr, *count = nullptr;
    int rows = 0;
};

// nmpc_contact_track_batch under the explicit `push` (refused as nmpc_contact_set_push refuses it) in place of whatever is
// attached to the handle, which is neither read nor rewritten: the track launch of a plant-mode rollout that pushes as a force.
// `windows` (if any) replace the window of `push` as the attached ones replace the attached push's; they are stated in a count
// in which the call's substep 0 is substep s0.
int contact_track_pushed(void* handle, int B, int n_steps, int n_sub, float dt, const nmpc_contact_cfg* cfg, float* q, float* v,
                         const float* tau_ff, const float* A, int a_rows, float kp, float kd, float* Q, float* V, int qv_rows,
                         const int* skip, int skip_mask, const nmpc_push_cfg& push, const PushWindows& windows, long long s0,
                         void* stream);

// nullptr if the handle's tree can serve the articulated momentum model of a whole-body solver on `device` (-1: any device): 18
// joints -- the coordinates of model 2 -- and some mass; otherwise the text nmpc_last_error gives
const char* momentum_refusal(void* handle, int device);

// total mass of the handle's tree (a handle momentum_refusal accepts)
float tree_mass(void* handle);

// the momentum pass of one SQP iteration (nmpc_torque_centroidal.hip.inc): the momentum records (nmpc_wb_momentum.hpp) of the B (N + 1)
// nodes of the iterate X [B][N+1][42], read through the warm-start shift, into rec; launched on the caller's current device.
// Left out, as the linearisation leaves them out: problems with skip[b] & skip_mask != 0, and, with `done` given (dev: the
// finished flag of problem 0, that of problem b `done_stride` words further on), problems whose flag is set
int momentum_records(void* handle, int B, int N, int shift, const float* X, const int* skip, int skip_mask, const int* done,
                     size_t done_stride, float* rec, void* stream);

}  // namespace nmpc_torque
