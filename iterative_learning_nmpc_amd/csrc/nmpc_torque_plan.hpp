// nmpc_torque_plan.hpp -- the one thing the rollout host code (nmpc_api.hip) asks of the torque layer (nmpc_torque.hip) beyond
// its C-ABI: whether a label launch with these arguments would be refused, so that a rollout refuses before it launches anything.
#pragma once

namespace nmpc_torque {

// nullptr if nmpc_plan_actions_batch accepts (handle, n_steps, zoh, kp) and the handle lives on `device` (-1: any device);
// otherwise the text nmpc_torque_last_error would give
const char* plan_actions_refusal(void* handle, int n_steps, const int* zoh, float kp, int device);

}  // namespace nmpc_torque
