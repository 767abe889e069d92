// mjs_policy.h — the tasks' scripted demonstration policies on the device: flat observations in, actions out, one env per lane.
// Replaces the per-task policy closures that scripts/demonstration_collection.py:303-345 drives (point_reach.py:227-240,
// robot_reach.py:222-253, robot_push_button.py:231-300). float64 throughout, no LDS, no atomics. The policy noise of the reference
// comes from the global np.random (no env stream, no parity contract): the caller supplies the standard-normal draws.
#pragma once
#include "mjs_kernel_common.h"
#include "mjs_reach.h"
#include "mjs_button.h"
#include "mjs_pointmass.h"

namespace pol {

struct PolicyParams {
  int N;
  int task;         // MJS_TASK_* (Planar-Push is refused on the host: its "policy" is a keyboard teleop)
  int action_type;  // MJS_ACTION_* (Button-Push)
  int obs_dim;      // row stride of obs
  int act_dim;      // row stride of actions
  double noise;     // 0: none
  const double* obs;  // [N, obs_dim], layout: mjs_obs_dim()
  const double* z;    // standard-normal draws [N, 2] (Pointmass) / [N, 3] (Robot-Reach) or nullptr
  double* actions;    // [N, act_dim]
  uint8_t* ik_ok;     // [N] or nullptr
};

MJS_DEV double max_abs3(const double* d) { return fmax(fmax(fabs(d[0]), fabs(d[1])), fabs(d[2])); }

// point_reach.py:227-240
MJS_DEV void pointmass_policy(const PolicyParams& p, int i) {
  const double* o = p.obs + (size_t)i * p.obs_dim;  // pointmass/position(2), goal_position(2)
  double a0 = o[2] - o[0], a1 = o[3] - o[1];        // :233 action = target_position - current_position
  if (p.z && p.noise > 0) {                         // :234-235 action *= 1 + np.random.normal(0, noise, action.shape)
    a0 *= 1 + p.noise * p.z[(size_t)i * 2 + 0];
    a1 *= 1 + p.noise * p.z[(size_t)i * 2 + 1];
  }
  // :236 action *= 1 / np.max(np.abs(action)) * MAX_STEP_SIZE. The reference divides by zero when the mass sits on the goal;
  // the host mirror clamps the maximum with 1e-300 (the action is then 0, not NaN), and so does this
  const double scale = MJS_PM_MAX_STEP_SIZE / fmax(fmax(fabs(a0), fabs(a1)), 1e-300);
  p.actions[(size_t)i * p.act_dim + 0] = a0 * scale;
  p.actions[(size_t)i * p.act_dim + 1] = a1 * scale;
  if (p.ik_ok) p.ik_ok[i] = 1;
}

// robot_reach.py:240-249
MJS_DEV void reach_policy(const PolicyParams& p, int i) {
  const double* o = p.obs + (size_t)i * p.obs_dim;  // ur5e/tcp_position(3), ur5e/joint_configuration(6), target_position(3)
  double d[3];
  for (int k = 0; k < 3; k++) d[k] = o[9 + k] - o[k];  // :241 difference = target_pose - robot_pose[:3]
  if (p.z && p.noise != 0)
    for (int k = 0; k < 3; k++) d[k] += p.noise * p.z[(size_t)i * 3 + k];  // :244 difference += np.random.normal(0, noise_level, size=3)
  // :247-248 "move at most 0.5m/s", as written there: the threshold 0.5 is compared with a DISTANCE (not with 0.5 * control_timestep),
  // and a difference above it is scaled to 0.5 * control_timestep
  const double m = max_abs3(d);
  if (m > 0.5)
    for (int k = 0; k < 3; k++) d[k] = d[k] * 0.5 / m * MJS_RR_CONTROL_DT;
  for (int k = 0; k < 3; k++) p.actions[(size_t)i * p.act_dim + k] = o[k] + d[k];  // :249
  if (p.ik_ok) p.ik_ok[i] = 1;
}

// robot_push_button.py:236-297
MJS_DEV void button_policy(const PolicyParams& p, int i) {
  const double* o = p.obs + (size_t)i * p.obs_dim;  // ur5e/joint_configuration(6), ur5e/tcp_position(3), switch/position(3), switch/active(1)
  double q[6], tcp[3], sw[3], goal[3];
  for (int k = 0; k < 6; k++) q[k] = o[k];
  for (int k = 0; k < 3; k++) { tcp[k] = o[6 + k]; sw[k] = o[9 + k]; }
  const bool active = o[12] > 0.5;
  const double dx = tcp[0] - sw[0], dy = tcp[1] - sw[1];
  const double planar = sqrt(dx * dx + dy * dy);  // np.linalg.norm(robot_position[:2] - target_position[:2])
  if (active) {  // :249-250, :276-280 phase 3: to the end pose, lifting first while still near the switch
    goal[0] = MJS_BP_ROBOT_END_POS[0];
    goal[1] = MJS_BP_ROBOT_END_POS[1];
    goal[2] = planar < 0.05 ? sw[2] + 0.1 : MJS_BP_ROBOT_END_POS[2];
  } else if (tcp[2] > sw[2] && planar < 0.01) {  // :251-256, :272-274 phase 2: straight down onto the switch
    goal[0] = sw[0]; goal[1] = sw[1]; goal[2] = sw[2];
  } else {  // :261-270 phase 1: hover 5 cm above the switch, rising in place first when below its top + 2 cm
    const bool too_low = tcp[2] < sw[2] + 0.02;
    goal[0] = too_low ? tcp[0] : sw[0];
    goal[1] = too_low ? tcp[1] : sw[1];
    goal[2] = sw[2] + 0.05;
    // (:264-265 write the goal into the array that also holds the robot position, so the reference's own difference is zero on
    // this branch and its rise is not speed-limited; the host mirror RobotPushButtonTask.demonstration_actions limits it like
    // every other branch, the oracle tests pin that, and this kernel follows the host mirror)
  }
  // :283-288 MAX_SPEED * control_timestep clamp on the largest component
  double d[3];
  for (int k = 0; k < 3; k++) d[k] = goal[k] - tcp[k];
  const double m = max_abs3(d), limit = 0.5 * MJS_RR_CONTROL_DT;
  const double scale = m > limit ? limit / fmax(m, 1e-300) : 1.0;
  double target[3];
  for (int k = 0; k < 3; k++) target[k] = tcp[k] + d[k] * scale;
  double* a = p.actions + (size_t)i * p.act_dim;
  bool found = true;
  if (p.action_type == MJS_ACTION_ABS_JOINT) {  // :291-294 get_joint_positions_from_tcp_pose(action + TOP_DOWN_QUATERNION, current joints)
    double out[6];
    for (int k = 0; k < 6; k++) out[k] = q[k];
    found = rr::tcp_pose_to_joints(target, q, out);
    // no solution: the reference raises; the env holds its joints (what mjs_ur5e_tcp_to_joints returns too) and ik_ok says so
    for (int k = 0; k < 6; k++) a[k] = found ? out[k] : q[k];
    a[6] = 0.0;  // :297 the gripper stays closed
  } else {
    for (int k = 0; k < 3; k++) a[k] = target[k];
    a[3] = 0.0;
  }
  if (p.ik_ok) p.ik_ok[i] = found;
}

__global__ __launch_bounds__(64) void kernel(PolicyParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.N) return;
  if (p.task == MJS_TASK_POINTMASS_REACH) pointmass_policy(p, i);
  else if (p.task == MJS_TASK_ROBOT_REACH) reach_policy(p, i);
  else button_policy(p, i);
}

}  // namespace pol
