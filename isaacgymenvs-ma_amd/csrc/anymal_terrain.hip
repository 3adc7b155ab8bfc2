// anymal_terrain.hip — AnymalTerrain's kernels (anymal_terrain_task.hpp) and their entry points, in a translation
// unit (and so a code object) of its own, linked last, as height_scan.hip is: the code objects before it are what they
// are without it.
#include "common.hpp"
#include "anymal_terrain_task.hpp"

namespace {
using mgi::fail;

int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MG_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
  return MG_OK;
}

// the shared argument check: a bound free-base 12-DOF sim whose bodies hold the task's rows, every tensor named
int args_ok(const mg_sim* sim, const mg_anymal_terrain_params* ap, const mg_anymal_terrain_views* v,
            const mg_task_buffers* tb, const char* who) {
  const std::string w(who);
  if (!sim || !ap || !v || !tb) return fail(MG_EINVAL, w + ": bad arguments");
  if (!sim->bound) return fail(MG_EINVAL, w + ": sim not bound");
  const mg_model& m = sim->host_model;
  if (m.fixed_base || m.obj_type || m.num_nodes - 1 != MG_ANYMAL_DOFS)
    return fail(MG_EINVAL, w + ": needs a free-base model of 12 DOFs without a free object");
  if (ap->num_bodies != m.num_bodies) return fail(MG_EINVAL, w + ": num_bodies does not match the sim's model");
  bool rows = ap->base_body >= 0 && ap->base_body < m.num_bodies;
  for (int k = 0; k < 4; k++) {
    rows = rows && ap->knee_body[k] >= 0 && ap->knee_body[k] < m.num_bodies;
    rows = rows && ap->foot_body[k] >= 0 && ap->foot_body[k] < m.num_bodies;
    rows = rows && ap->hip_dof[k] >= 0 && ap->hip_dof[k] < MG_ANYMAL_DOFS;
  }
  if (!rows) return fail(MG_EINVAL, w + ": a base, knee or foot body or a hip DOF is out of range");
  if (!v->commands || !v->torques || !v->last_actions || !v->last_dof_vel || !v->feet_air_time || !v->episode_sums ||
      !v->terrain_levels || !v->terrain_types || !v->env_origins || !v->dof_actuation || !v->episode_out ||
      !v->partials || !v->reset_mark)
    return fail(MG_EINVAL, w + ": a tensor of mg_anymal_terrain_views is NULL");
  if (ap->custom_origins && (!v->terrain_origins || ap->env_rows < 1 || ap->env_cols < 1))
    return fail(MG_EINVAL, w + ": custom_origins needs terrain_origins of at least 1 x 1 maps");
  if (ap->hf_heights && (ap->hf_nx < 2 || ap->hf_ny < 2 || !(ap->hf_dx > 0.0f)))
    return fail(MG_EINVAL, w + ": the scan's field needs nx, ny >= 2 and a positive dx");
  return MG_OK;
}

int blocks_of(int n) { return (n + mgat::kEnvs - 1) / mgat::kEnvs; }
}  // namespace

extern "C" {

size_t mg_anymal_terrain_params_sizeof(void) { return sizeof(mg_anymal_terrain_params); }
size_t mg_anymal_terrain_views_sizeof(void) { return sizeof(mg_anymal_terrain_views); }

int mg_anymal_terrain_pre(mg_sim* sim, const mg_anymal_terrain_params* ap, const mg_anymal_terrain_views* views,
                          const mg_task_buffers* tb, void* stream) {
  if (int rc = args_ok(sim, ap, views, tb, "mg_anymal_terrain_pre")) return rc;
  if (!tb->actions || !sim->views.dof_state) return fail(MG_EINVAL, "mg_anymal_terrain_pre: needs actions and dof_state");
  if (sim->views.dof_actuation != views->dof_actuation)
    return fail(MG_EINVAL, "mg_anymal_terrain_pre: views.dof_actuation is not the buffer the sim has bound as "
                           "dof_actuation");
  if (sim->n == 0) return MG_OK;
  const long long total = (long long)sim->n * MG_ANYMAL_DOFS;
  hipLaunchKernelGGL(mgat::k_at_pre, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *ap,
                     tb->actions, tb->actions_out, (const float*)sim->views.dof_state, views->dof_actuation,
                     views->torques, total);
  return launched("mg_anymal_terrain_pre");
}

int mg_anymal_terrain_post(mg_sim* sim, const mg_anymal_terrain_params* ap, const mg_anymal_terrain_views* views,
                           const mg_task_buffers* tb, const mg_state_views* state, void* stream) {
  if (int rc = args_ok(sim, ap, views, tb, "mg_anymal_terrain_post")) return rc;
  if (!tb->actions || !tb->obs || !tb->rew || !tb->reset || !tb->progress || !tb->timeout)
    return fail(MG_EINVAL, "mg_anymal_terrain_post: needs actions, obs, rew, reset, progress and timeout");
  const mg_state_views& s = state ? *state : sim->views;
  if (!s.root_states || !s.dof_state || !s.net_contact_forces)
    return fail(MG_EINVAL, "mg_anymal_terrain_post: needs root_states, dof_state and net_contact_forces");
  if (sim->n == 0) return MG_OK;
  mgat::State st{s.root_states, s.dof_state, s.net_contact_forces};
  const int blocks = blocks_of(sim->n);
  hipLaunchKernelGGL(mgat::k_at_post, dim3(blocks), dim3(64), 0, (hipStream_t)stream, *ap, *views, *tb, st, sim->n);
  hipLaunchKernelGGL(mgat::k_at_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, *ap, *views, blocks, sim->n);
  return launched("mg_anymal_terrain_post");
}

int mg_anymal_terrain_reset_idx(mg_sim* sim, const mg_anymal_terrain_params* ap,
                                const mg_anymal_terrain_views* views, const mg_task_buffers* tb, const int32_t* ids,
                                int32_t n, int32_t update_levels, void* stream) {
  if (int rc = args_ok(sim, ap, views, tb, "mg_anymal_terrain_reset_idx")) return rc;
  if (n < 0 || (n > 0 && !ids) || !tb->reset || !tb->progress || !sim->views.root_states || !sim->views.dof_state)
    return fail(MG_EINVAL, "mg_anymal_terrain_reset_idx: bad arguments");
  if (n == 0 || sim->n == 0) return MG_OK;
  mg_task_buffers t = *tb;
  t.step_counter = tb->step_counter | (1ull << 62);   // the manual-reset stream, as mg_reset_idx
  mgat::State st{sim->views.root_states, sim->views.dof_state, sim->views.net_contact_forces};
  const int blocks = blocks_of(sim->n);
  hipLaunchKernelGGL(mgat::k_at_mark, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, views->reset_mark, ids,
                     n, sim->n);
  hipLaunchKernelGGL(mgat::k_at_reset_marked, dim3(blocks), dim3(64), 0, (hipStream_t)stream, *ap, *views, t, st,
                     update_levels, sim->n);
  hipLaunchKernelGGL(mgat::k_at_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, *ap, *views, blocks, sim->n);
  return launched("mg_anymal_terrain_reset_idx");
}

}  // extern "C"
