// swing_ref_shim.cpp -- TEST INFRASTRUCTURE ONLY (see oracle/hmpc_oracle.h).
//
// Drives the reference's OWN swing-leg controller, compiled UNMODIFIED from the reference checkout by oracle/Makefile into
// oracle/_ref/libswing_ref.so:
//   src/common/SwingLegController.cpp    updateSwingLeg (foot position, sub-phase, timer, touchdown point, Bezier target), computeIK,
//                                        setDesiredJointState
//   ConvexMPC/GaitGenerator.cpp, ConvexMPC/ConvexMPCLocomotion.cpp, src/common/LegController.cpp, FootSwingTrajectory.cpp,
//   DesiredCommand.cpp                   (what it reads, and run() + updateCommand for whole ticks)
// against the Eigen stand-in oracle/mini_eigen and the placeholder boost/lcm headers oracle/ref_stubs.
//
// What this file supplies instead of reference code:
//   * setup_problem / update_problem_data / get_solution / update_solver_settings (convexMPC_interface.h): the arguments are dropped and
//     get_solution answers from a vector the test supplies (swr_set_solution);
//   * the object graph of ControlFSMData that the ROS main.cpp builds, plus per instance a Gait and a swingLegController initialised
//     through the reference's initSwingLegController;
//   * setters and getters.  Nothing here computes a quantity under test.
//
// The standard headers are included first, each once, so that the `#define private public` window below opens none of them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <unistd.h>

// swingLegController keeps its state private (SwingLegController.h:50-76), and so does the FootSwingTrajectory it holds.  The reference's
// translation units are compiled without this; only this window sees the members (access specifiers do not change layout).
#define private public
#include "../include/common/SwingLegController.h"
#undef private
#include "ConvexMPCLocomotion.h"
#include "convexMPC_interface.h"

namespace {
double g_solution[12 * K_MAX_GAIT_SEGMENTS];
}

extern "C" void setup_problem(double, int, double, double) {}
extern "C" void update_problem_data(double *, double *, double *, double *, double *, double *, double, double *, double *, double *, int *) {}
extern "C" double get_solution(int index) { return g_solution[index]; }
extern "C" void update_solver_settings(int, double, double, double, double, double) {}

struct SwingRef {
  Biped biped;
  LowlevelState lowState;
  LowlevelCmd lowCmd;
  StateEstimate se;
  LegController *legs;
  StateEstimatorContainer *estimator;
  DesiredStateCommand *command;
  ControlFSMData fsm;
  Gait *gait;
  swingLegController swing;
  ConvexMPCLocomotion *mpc;  // whole ticks only (swr_create_run)
};

static SwingRef *make_graph(double dt) {
  SwingRef *c = new SwingRef();
  memset(&c->se, 0, sizeof c->se);
  c->legs = new LegController(c->biped);
  c->estimator = new StateEstimatorContainer(&c->lowState, c->legs->data, &c->se);
  c->command = new DesiredStateCommand(&c->se, dt);
  c->fsm._biped = &c->biped;
  c->fsm._stateEstimator = c->estimator;
  c->fsm._legController = c->legs;
  c->fsm._desiredStateCommand = c->command;
  c->fsm._interface = nullptr;
  c->fsm._lowCmd = &c->lowCmd;
  c->fsm._lowState = &c->lowState;
  // LegControllerCommand::zero() declares two locals where it means kptoe / kdtoe (LegController.cpp:19-20): the members start undefined
  for (int leg = 0; leg < 2; ++leg) c->legs->commands[leg].kptoe = 0, c->legs->commands[leg].kdtoe = 0;
  c->gait = nullptr;
  c->mpc = nullptr;
  return c;
}

extern "C" {

void swr_set_solution(const double *sol, int n) { memcpy(g_solution, sol, sizeof(double) * n); }

// a Gait(n_segments, offsets, durations) and a swingLegController initialised as run() does it (ConvexMPCLocomotion.cpp:68)
SwingRef *swr_create(int n_segments, int off0, int off1, int dur0, int dur1, double dtSwing) {
  SwingRef *c = make_graph(0.001);
  c->gait = new Gait(n_segments, Vec2<int>(off0, off1), Vec2<int>(dur0, dur1), "swing_ref");
  c->swing.initSwingLegController(&c->fsm, c->gait, dtSwing);
  return c;
}
// a ConvexMPCLocomotion(dt, iterations_between_mpc) for whole ticks; its constructor opens "foot_pos.txt" in the working directory
SwingRef *swr_create_run(double dt, int iterations_between_mpc, const char *scratch_dir) {
  char cwd[4096];
  if (!getcwd(cwd, sizeof cwd)) return nullptr;
  if (scratch_dir && chdir(scratch_dir) != 0) return nullptr;
  SwingRef *c = make_graph(dt);
  c->mpc = new ConvexMPCLocomotion(dt, iterations_between_mpc);
  if (scratch_dir && chdir(cwd) != 0) return nullptr;
  return c;
}
void swr_destroy(SwingRef *c) {
  if (!c) return;
  delete c->mpc;
  delete c->gait;
  delete c->command;
  delete c->estimator;
  delete c->legs;
  delete c;
}

// StateEstimate fields (StateEstimatorContainer.h); rBody row-major, world -> body
void swr_set_state(SwingRef *c, const double *position, const double *vWorld, const double *omegaWorld, const double *orientation,
                   const double *rpy, const double *rBody) {
  for (int i = 0; i < 3; ++i) {
    c->se.position[i] = position[i], c->se.vWorld[i] = vWorld[i], c->se.omegaWorld[i] = omegaWorld[i], c->se.rpy[i] = rpy[i];
    for (int j = 0; j < 3; ++j) c->se.rBody(i, j) = rBody[3 * i + j];
  }
  for (int i = 0; i < 4; ++i) c->se.orientation[i] = orientation[i];
  c->se.vBody = c->se.rBody * c->se.vWorld;  // PositionVelocityEstimator.cpp:10-11 (run() reads it for v_abs, which nothing uses)
}
void swr_set_command(SwingRef *c, const double *stateDes12) {
  for (int i = 0; i < 12; ++i) c->command->data.stateDes[i] = stateDes12[i];
}
// the reference's own LegController::updateData (LegController.cpp:42-55) on motor angles (MotorState::q is float)
void swr_update_leg_data_from_motors(SwingRef *c, const float *q10) {
  for (int i = 0; i < 10; ++i) c->lowState.motorState[i].q = q10[i], c->lowState.motorState[i].dq = 0.f, c->lowState.motorState[i].tauEst = 0.f;
  c->legs->updateData(&c->lowState);
}
// writes data[leg].q as stored (a tick without HMPC_TICK_LEG_Q_MOTOR); data[leg].p and the Jacobians stay as the last updateData left them
void swr_poke_leg_q(SwingRef *c, const double *q10) {
  for (int leg = 0; leg < 2; ++leg)
    for (int j = 0; j < 5; ++j) c->legs->data[leg].q(j) = q10[5 * leg + j];
}
void swr_get_leg(SwingRef *c, int leg, double *q5, double *p3) {
  for (int j = 0; j < 5; ++j) q5[j] = c->legs->data[leg].q(j);
  for (int i = 0; i < 3; ++i) p3[i] = c->legs->data[leg].p(i);
}

// gait.setIterations(ticks_per_step, cur), then updateSwingLeg() `updates` times (run() calls it once per foot)
void swr_update(SwingRef *c, int ticks_per_step, int cur, int updates) {
  c->gait->setIterations(ticks_per_step, cur);
  for (int u = 0; u < updates; ++u) c->swing.updateSwingLeg();
}
// the public computeIK on a body-frame target; data[leg].q(2), q(3) are poked first (it reads them for joint 4)
void swr_compute_ik(SwingRef *c, const double *pFoot_b3, int leg, double q2, double q3, double *q5) {
  c->legs->data[leg].q(2) = q2, c->legs->data[leg].q(3) = q3;
  Vec3<double> p(pFoot_b3[0], pFoot_b3[1], pFoot_b3[2]);
  Eigen::Matrix<double, 5, 1> q;
  c->swing.computeIK(p, q, leg);
  for (int j = 0; j < 5; ++j) q5[j] = q(j);
}

// the private state of the swing controller (SwingLegController.h:50-67), per leg: layout
//   [0] swingTimes, [1] firstSwing, [2..4] _p0, [5..7] _pf, [8] swingStates, [9..11] pFoot_w, [12..14] pFoot_b, [15..17] vFoot_b,
//   and the trajectory's public getPosition() [18..20] / getVelocity() [21..23] (world frame; read only)
void swr_get_swing(SwingRef *c, int leg, double *row24) {
  swingLegController &s = c->swing;
  row24[0] = s.swingTimes[leg], row24[1] = s.firstSwing[leg] ? 1.0 : 0.0, row24[8] = s.swingStates[leg];
  for (int i = 0; i < 3; ++i) {
    row24[2 + i] = s.footSwingTrajectory[leg]._p0[i], row24[5 + i] = s.footSwingTrajectory[leg]._pf[i];
    row24[9 + i] = s.pFoot_w[leg][i], row24[12 + i] = s.pFoot_b[leg][i], row24[15 + i] = s.vFoot_b[leg][i];
  }
  const Vec3<double> p = s.footSwingTrajectory[leg].getPosition(), v = s.footSwingTrajectory[leg].getVelocity();
  for (int i = 0; i < 3; ++i) row24[18 + i] = p[i], row24[21 + i] = v[i];
}
void swr_set_swing(SwingRef *c, int leg, const double *row24) {
  swingLegController &s = c->swing;
  s.swingTimes[leg] = row24[0], s.firstSwing[leg] = row24[1] != 0.0, s.swingStates[leg] = row24[8];
  for (int i = 0; i < 3; ++i) {
    s.footSwingTrajectory[leg]._p0[i] = row24[2 + i], s.footSwingTrajectory[leg]._pf[i] = row24[5 + i];
    s.pFoot_w[leg][i] = row24[9 + i], s.pFoot_b[leg][i] = row24[12 + i], s.vFoot_b[leg][i] = row24[15 + i];
  }
}
// commands[leg]: [0..4] qDes, [5..9] qdDes, [10..12] pDes, [13..15] vDes, [16..20] diag kpJoint, [21..25] diag kdJoint,
//   [26..31] feedforwardForce, [32] kptoe, [33] kdtoe
void swr_get_command(SwingRef *c, int leg, double *out34) {
  const LegControllerCommand &m = c->legs->commands[leg];
  for (int j = 0; j < 5; ++j) out34[j] = m.qDes(j), out34[5 + j] = m.qdDes(j), out34[16 + j] = m.kpJoint(j, j), out34[21 + j] = m.kdJoint(j, j);
  for (int i = 0; i < 3; ++i) out34[10 + i] = m.pDes(i), out34[13 + i] = m.vDes(i);
  for (int i = 0; i < 6; ++i) out34[26 + i] = m.feedforwardForce(i);
  out34[32] = m.kptoe, out34[33] = m.kdtoe;
}
void swr_set_q_des(SwingRef *c, const double *q10) {
  for (int leg = 0; leg < 2; ++leg)
    for (int j = 0; j < 5; ++j) c->legs->commands[leg].qDes(j) = q10[5 * leg + j];
}

// a whole tick as FSMState_Walking::run makes it (FSMState_Walking.cpp:36-39): setGaitNum, run, updateCommand; the five float fields
// of the ten LowlevelCmd::motorCmd as [10][5] = q, dq, Kp, Kd, tau
void swr_run_tick(SwingRef *c, int gaitNumber, float *cmd50) {
  c->mpc->setGaitNum(gaitNumber);
  c->mpc->run(c->fsm);
  c->legs->updateCommand(&c->lowCmd);
  for (int i = 0; i < 10; ++i) {
    const MotorCmd &m = c->lowCmd.motorCmd[i];
    cmd50[5 * i] = m.q, cmd50[5 * i + 1] = m.dq, cmd50[5 * i + 2] = m.Kp, cmd50[5 * i + 3] = m.Kd, cmd50[5 * i + 4] = m.tau;
  }
}
// what the reference's updateCommand (LegController.cpp:57-99) makes of feedforwardForce = f on BOTH legs at the present leg data:
// tau = (float)(J_force_moment' f).  The commands are put back as they were and a scratch LowlevelCmd receives the result.
void swr_tau_of(SwingRef *c, const double *f_ff12, float *tau10) {
  LegControllerCommand keep[2] = {c->legs->commands[0], c->legs->commands[1]};
  LowlevelCmd scratch;
  for (int leg = 0; leg < 2; ++leg)
    for (int i = 0; i < 6; ++i) c->legs->commands[leg].feedforwardForce(i) = f_ff12[6 * leg + i];
  c->legs->updateCommand(&scratch);
  for (int i = 0; i < 10; ++i) tau10[i] = scratch.motorCmd[i].tau;
  c->legs->commands[0] = keep[0], c->legs->commands[1] = keep[1];
}
}  // extern "C"
