// render.hpp — a pinhole ray caster over an env's collision geometry (include/migym.h: mg_render).
//
// Two launches on the caller's stream, no host synchronisation, no atomics:
//   k_render_setup  one 16-lane team per (selected env, actor): kinematics-only FK from root_states / dof_state (the
//                   chain walk and conventions of team_fk_crba in dynamics_tensors.hpp: node 0 is the root row, DOF j
//                   is node j + 1, a lane owns the nodes tl, tl + 16, tl + 32), then one 16-float record per
//                   primitive into the caller's scratch: world rotation 9 (row-major), world position 3, size 3, one
//                   word (type | colour index << 8).  Primitive order = the id image's ids: the actors' geoms, the
//                   free object and the goal (hand tasks), the caller's extra boxes, the ground plane z = 0.
//   k_render_trace  one block per (selected env, tile of kTile consecutive pixels): the env's records are staged in
//                   LDS (64 B each, kMaxPrims at most), each lane traces its pixel against every primitive.  The
//                   primitive index is uniform across the wave, so the per-type branch is uniform and the hull's
//                   planes are read at uniform addresses.  Two conservative culls: a wave whose rays all pass a
//                   primitive's (grown) bounding sphere skips it, and one whose rays all miss the hull's (grown)
//                   bounding box skips its planes.  Nearest t > kTmin wins, ties go to the lower id.  Depth
//                   and id stores are consecutive across the wave; RGB goes through LDS so that every store
//                   instruction of a wave writes consecutive bytes.
// The image shows collision geometry: no visual meshes, textures, shadows or anti-aliasing; the output is a
// deterministic function of the state.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "device_math.hpp"

namespace mgrd {
using namespace mg;

constexpr int kTeam = 16;            // lanes per actor (setup)
constexpr int kTeams = 64 / kTeam;   // actors per setup block
constexpr int kRec = 16;             // floats per primitive record
constexpr int kMaxPrims = 512;       // records staged in LDS: 32 KB
constexpr int kTile = 256;           // pixels (lanes) per trace block
constexpr int kNone = 7;             // record type of an env id outside 0..N-1: nothing to hit (the image is sky)
constexpr float kTmin = 1e-4f;
// colour indices of the record word: 0..7 the body palette, then object, goal, extra box, the ground's two greys, sky
constexpr int kColObject = 8, kColGoal = 9, kColBox = 10, kColGround = 11, kColSky = 13;
__constant__ float kPalette[14][3] = {
    {0.90f, 0.30f, 0.25f}, {0.25f, 0.60f, 0.90f}, {0.35f, 0.75f, 0.35f}, {0.95f, 0.75f, 0.20f},
    {0.65f, 0.40f, 0.85f}, {0.20f, 0.75f, 0.75f}, {0.95f, 0.55f, 0.25f}, {0.75f, 0.75f, 0.78f},
    {0.95f, 0.85f, 0.30f}, {0.40f, 0.95f, 0.55f}, {0.90f, 0.45f, 0.75f}, {0.55f, 0.55f, 0.55f},
    {0.75f, 0.75f, 0.75f}, {0.53f, 0.73f, 0.92f}};

struct SetupArgs {
  const mg_model* m;         // device
  const float* root;         // bound root_states
  const float* dof;          // bound dof_state
  const int32_t* env_ids;    // (n_sel) or nullptr = the first n_sel envs
  const float* boxes;        // (n_env, K, 10) or nullptr
  float* scratch;            // (n_sel, P, 16)
  int n_sel, n_env, A, K, P, rows_per_env;
};

__device__ __forceinline__ M3 unit_quat_to_mat(const float* q) {
  const float qn = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  return quat_to_mat(q[0] * qn, q[1] * qn, q[2] * qn, q[3] * qn);
}

__device__ __forceinline__ void put_record(float* rec, const M3& R, V3 p, float s0, float s1, float s2, int type,
                                           int colour) {
  float4* o = reinterpret_cast<float4*>(rec);
  o[0] = make_float4(R.m[0][0], R.m[0][1], R.m[0][2], R.m[1][0]);
  o[1] = make_float4(R.m[1][1], R.m[1][2], R.m[2][0], R.m[2][1]);
  o[2] = make_float4(R.m[2][2], p.x, p.y, p.z);
  o[3] = make_float4(s0, s1, s2, __uint_as_float((unsigned)type | ((unsigned)colour << 8)));
}

__device__ __forceinline__ M3 identity3() {
  M3 I;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) I.m[a][b] = a == b ? 1.0f : 0.0f;
  return I;
}

__global__ __launch_bounds__(64) void k_render_setup(SetupArgs s) {
  extern __shared__ float frames[];   // kTeams x num_nodes x 12: every node's world rotation and origin
  const mg_model* __restrict__ m = s.m;
  const int team = threadIdx.x / kTeam, tl = threadIdx.x % kTeam;
  const int t = blockIdx.x * kTeams + team;
  const bool live = t < s.n_sel * s.A;
  const int sel = live ? t / s.A : 0, a = live ? t - sel * s.A : 0;
  const int e = s.env_ids ? s.env_ids[sel] : sel;
  const bool valid = live && e >= 0 && e < s.n_env;
  const int nn = m->num_nodes, nG = m->num_geoms;
  float* fr = frames + (size_t)12 * nn * team;
  const float* root = s.root + (size_t)13 * ((size_t)(valid ? e : 0) * s.rows_per_env + a);
  const float* dof = s.dof + (size_t)2 * (nn - 1) * ((size_t)(valid ? e : 0) * s.A + a);
  if (valid) {
    const M3 Rr = unit_quat_to_mat(root + 3);
    const V3 x0 = ld3(root);
    for (int node = tl; node < nn; node += kTeam) {
      unsigned long long path = 0;   // the node's chain below the root (parent < child: ascending bits = root first)
      for (int k = node; k > 0; k = m->parent[k]) path |= 1ull << k;
      M3 R = Rr;
      V3 x = x0;
      for (; path; path &= path - 1) {
        const int k = __builtin_ctzll(path);
        const M3 Rp0 = mul(R, unit_quat_to_mat(m->r0[k]));
        const V3 tp = mul(R, ld3(m->t[k]));
        const V3 ax = ld3(m->axis[k]);
        const float qk = dof[2 * (k - 1)];
        if (m->jtype[k] == MG_JT_HINGE) {
          R = mul(Rp0, axis_angle(ax, qk));
          x = x + tp;
        } else {
          R = Rp0;
          x = x + tp + mul(Rp0, ax) * qk;
        }
      }
      float* f = fr + 12 * node;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) f[3 * i + j] = R.m[i][j];
      f[9] = x.x; f[10] = x.y; f[11] = x.z;
    }
  }
  __syncthreads();
  if (!live) return;
  float* out = s.scratch + (size_t)kRec * s.P * sel;
  for (int g = tl; g < nG; g += kTeam) {
    float* rec = out + (size_t)kRec * (a * nG + g);
    if (!valid) {
      put_record(rec, identity3(), v3(0, 0, 0), 0, 0, 0, kNone, 0);
      continue;
    }
    const float* f = fr + 12 * m->geom_node[g];
    M3 Rn;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) Rn.m[i][j] = f[3 * i + j];
    const M3 Rw = mul(Rn, unit_quat_to_mat(m->geom_quat[g]));
    const V3 pw = ld3(f + 9) + mul(Rn, ld3(m->geom_pos[g]));
    put_record(rec, Rw, pw, m->geom_size[g][0], m->geom_size[g][1], m->geom_size[g][2], m->geom_type[g],
               m->geom_body[g] & 7);
  }
  if (a != 0) return;
  // the env's own primitives, by the team of its actor 0
  int base = s.A * nG;
  if (m->obj_type != 0) {   // root rows 1 (object) and 2 (goal) of the env
    if (tl < 2) {
      if (valid) {
        const float* row = s.root + (size_t)13 * ((size_t)e * s.rows_per_env + 1 + tl);
        put_record(out + (size_t)kRec * (base + tl), unit_quat_to_mat(row + 3), ld3(row), m->obj_size[0], m->obj_size[1],
                   m->obj_size[2], m->obj_type, tl == 0 ? kColObject : kColGoal);
      } else {
        put_record(out + (size_t)kRec * (base + tl), identity3(), v3(0, 0, 0), 0, 0, 0, kNone, 0);
      }
    }
    base += 2;
  }
  for (int k = tl; k < s.K; k += kTeam) {
    float* rec = out + (size_t)kRec * (base + k);
    if (valid) {
      const float* b = s.boxes + (size_t)10 * ((size_t)e * s.K + k);
      put_record(rec, unit_quat_to_mat(b + 3), ld3(b), b[7], b[8], b[9], MG_GT_BOX, kColBox);
    } else {
      put_record(rec, identity3(), v3(0, 0, 0), 0, 0, 0, kNone, 0);
    }
  }
  if (tl == kTeam - 1)
    put_record(out + (size_t)kRec * (s.P - 1), identity3(), v3(0, 0, 0), 0, 0, 0, valid ? MG_GT_PLANE : kNone, kColGround);
}

struct TraceArgs {
  const float* scratch;      // (n_sel, P, 16)
  const mg_model* m;         // device: the hull's planes
  const float* root;
  const int32_t* env_ids;
  uint8_t* rgb;              // (n_sel, H, W, 3) or nullptr
  float* depth;              // (n_sel, H, W) or nullptr
  int32_t* ids;              // (n_sel, H, W) or nullptr
  int W, H, P, n_env, rows_per_env, follow, tiles;
  float tan_half;            // tan(fov_y / 2)
  float eye[3], tgt[3];      // offsets from the anchor
};

// of the two roots of a convex primitive (t0 <= t1), the nearest one beyond kTmin; +inf if neither is
__device__ __forceinline__ float near_root(float t0, float t1) {
  return t0 > kTmin ? t0 : (t1 > kTmin ? t1 : INFINITY);
}

// a sphere of radius r about c on the ray o + t d (|d| = 1), through the ray's closest point to the centre: the
// discriminant is r^2 - (distance)^2 with no cancellation between |o|^2-sized terms.  false = missed
__device__ __forceinline__ bool sphere_roots(V3 o, V3 d, float r, float* t0, float* t1) {
  const float a = dot(d, d);
  const float b = dot(o, d) / a;
  const V3 l = o - d * b;
  const float h2 = (r * r - dot(l, l)) / a;
  if (!(h2 >= 0.0f)) return false;
  const float h = sqrtf(h2);
  *t0 = -b - h;
  *t1 = -b + h;
  return true;
}
// the infinite cylinder of radius r about the z axis
__device__ __forceinline__ bool cylinder_roots(V3 o, V3 d, float r, float* t0, float* t1) {
  const float a = d.x * d.x + d.y * d.y;
  const float b = (o.x * d.x + o.y * d.y) / a;
  const float lx = o.x - b * d.x, ly = o.y - b * d.y;
  const float h2 = (r * r - (lx * lx + ly * ly)) / a;
  if (!(h2 >= 0.0f)) return false;
  const float h = sqrtf(h2);
  *t0 = -b - h;
  *t1 = -b + h;
  return true;
}

// One primitive in its own frame: the nearest hit beyond kTmin (or +inf) and its outward normal, local.
__device__ __forceinline__ float hit_primitive(int type, V3 o, V3 d, V3 sz, const mg_model* __restrict__ m, V3* n) {
  float t = INFINITY;
  *n = v3(0, 0, 1);
  if (type == MG_GT_SPHERE) {
    float t0, t1;
    if (sphere_roots(o, d, sz.x, &t0, &t1)) {
      t = near_root(t0, t1);
      *n = (o + d * t) * (1.0f / sz.x);
    }
  } else if (type == MG_GT_ELLIPSOID) {   // the unit sphere in the space scaled by the semi-axes (t is unchanged)
    const V3 os = v3(o.x / sz.x, o.y / sz.y, o.z / sz.z), ds = v3(d.x / sz.x, d.y / sz.y, d.z / sz.z);
    float t0, t1;
    if (sphere_roots(os, ds, 1.0f, &t0, &t1)) {
      t = near_root(t0, t1);
      const V3 p = os + ds * t;
      const V3 g = v3(p.x / sz.x, p.y / sz.y, p.z / sz.z);
      *n = g * (1.0f / sqrtf(dot(g, g)));
    }
  } else if (type == MG_GT_CAPSULE) {   // radius sz.x, half length sz.y along z: the side where |z| <= half, else a cap
    const float r = sz.x, h = sz.y;
    float t0, t1;
    if (cylinder_roots(o, d, r, &t0, &t1)) {
      if (t1 > kTmin && fabsf(o.z + t1 * d.z) <= h) t = t1;
      if (t0 > kTmin && fabsf(o.z + t0 * d.z) <= h) t = t0;
    }
    for (int c = 0; c < 2; c++) {
      const float sg = c == 0 ? 1.0f : -1.0f;
      const V3 oc = v3(o.x, o.y, o.z - sg * h);
      if (sphere_roots(oc, d, r, &t0, &t1)) {
        if (t1 > kTmin && t1 < t && (oc.z + t1 * d.z) * sg >= 0.0f) t = t1;
        if (t0 > kTmin && t0 < t && (oc.z + t0 * d.z) * sg >= 0.0f) t = t0;
      }
    }
    if (t < INFINITY) {
      const V3 p = o + d * t;
      *n = v3(p.x, p.y, p.z - fminf(fmaxf(p.z, -h), h)) * (1.0f / r);
    }
  } else if (type == MG_GT_CYLINDER) {   // capped: radius sz.x, half length sz.y along z
    const float r = sz.x, h = sz.y;
    float t0, t1;
    V3 nn = v3(0, 0, 1);
    if (cylinder_roots(o, d, r, &t0, &t1)) {
      float ts = INFINITY;
      if (t1 > kTmin && fabsf(o.z + t1 * d.z) <= h) ts = t1;
      if (t0 > kTmin && fabsf(o.z + t0 * d.z) <= h) ts = t0;
      if (ts < INFINITY) {
        t = ts;
        nn = v3((o.x + ts * d.x) / r, (o.y + ts * d.y) / r, 0.0f);
      }
    }
    for (int c = 0; c < 2; c++) {
      const float sg = c == 0 ? 1.0f : -1.0f;
      const float tc = (sg * h - o.z) / d.z;
      const float px = o.x + tc * d.x, py = o.y + tc * d.y;
      if (tc > kTmin && tc < t && px * px + py * py <= r * r) {
        t = tc;
        nn = v3(0, 0, sg);
      }
    }
    *n = nn;
  } else if (type == MG_GT_BOX) {   // slabs
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, hh[3] = {sz.x, sz.y, sz.z};
    float tn = -INFINITY, tf = INFINITY;
    int an = 0, af = 0;
    float dn = 0.0f, df = 0.0f;   // the ray direction along the entry / exit axis
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float inv = 1.0f / dd[k];
      const float ta = (-hh[k] - oo[k]) * inv, tb = (hh[k] - oo[k]) * inv;
      const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
      if (lo > tn) { tn = lo; an = k; dn = dd[k]; }
      if (hi < tf) { tf = hi; af = k; df = dd[k]; }
    }
    if (tn <= tf) {
      t = near_root(tn, tf);
      const bool entry = tn > kTmin;
      const int ax = entry ? an : af;
      const float sg = ((entry ? dn : df) > 0.0f) == entry ? -1.0f : 1.0f;
      *n = v3(ax == 0 ? sg : 0.0f, ax == 1 ? sg : 0.0f, ax == 2 ? sg : 0.0f);
    }
  } else if (type == MG_GT_CONVEX) {   // the model's hull, planes n.x <= dd inside: entry = the last front-facing
    float tn = -INFINITY, tf = INFINITY;   // plane crossed, exit = the first back-facing one
    int pn = 0, pf = 0;
    bool out = false;
    // cull: the hull lies inside the box of its half extents (geom_size, mg_model), here grown by 1e-4 relative + 1 um
    // so that fp32 rounding of the slab test can never reject a ray that touches the hull.  A wave none of whose
    // rays meets the box skips the plane loop.
    bool inbox;
    {
      const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, hh[3] = {sz.x, sz.y, sz.z};
      float bn = -INFINITY, bf = INFINITY;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float inv = 1.0f / dd[k], h = hh[k] * 1.0001f + 1e-6f;
        const float ta = (-h - oo[k]) * inv, tb = (h - oo[k]) * inv;
        bn = fmaxf(bn, fminf(ta, tb));
        bf = fminf(bf, fmaxf(ta, tb));
      }
      inbox = bn <= bf && bf > 0.0f;
    }
    const int np = inbox ? m->hull_num_planes : 0;
    for (int k = 0; k < np; k++) {
      const float* pl = m->hull_plane[k];
      const float den = pl[0] * d.x + pl[1] * d.y + pl[2] * d.z;
      const float dist = pl[3] - (pl[0] * o.x + pl[1] * o.y + pl[2] * o.z);
      if (den < 0.0f) {
        const float tk = dist / den;
        if (tk > tn) { tn = tk; pn = k; }
      } else if (den > 0.0f) {
        const float tk = dist / den;
        if (tk < tf) { tf = tk; pf = k; }
      } else if (dist < 0.0f) {
        out = true;
      }
    }
    if (np > 0 && !out && tn <= tf) {
      t = near_root(tn, tf);
      const float* pl = m->hull_plane[tn > kTmin ? pn : pf];
      *n = v3(pl[0], pl[1], pl[2]);
    }
  } else if (type == MG_GT_PLANE) {   // the plane z = 0 of the frame, seen from either side
    const float tp = -o.z / d.z;
    if (tp > kTmin) t = tp;
  }
  return t;
}

// squared radius of a sphere about the primitive's origin that holds it
__device__ __forceinline__ float bound_radius2(int type, V3 sz) {
  if (type == MG_GT_SPHERE) return sz.x * sz.x;
  if (type == MG_GT_CAPSULE) return (sz.x + sz.y) * (sz.x + sz.y);
  if (type == MG_GT_CYLINDER) return sz.x * sz.x + sz.y * sz.y;
  if (type == MG_GT_ELLIPSOID) {
    const float r = fmaxf(sz.x, fmaxf(sz.y, sz.z));
    return r * r;
  }
  return sz.x * sz.x + sz.y * sz.y + sz.z * sz.z;   // box, and the hull inside the box of its half extents
}

__device__ __forceinline__ unsigned to_u8(float c) { return (unsigned)fminf(fmaxf(floorf(255.0f * c + 0.5f), 0.0f), 255.0f); }

__global__ __launch_bounds__(kTile) void k_render_trace(TraceArgs a) {
  extern __shared__ float4 lds4[];   // P records, then 3 * kTile bytes of RGB
  float* rec = reinterpret_cast<float*>(lds4);
  unsigned char* pix = reinterpret_cast<unsigned char*>(lds4 + 4 * a.P);
  const int sel = blockIdx.x / a.tiles, tile = blockIdx.x - sel * a.tiles;
  {
    const float4* src = reinterpret_cast<const float4*>(a.scratch + (size_t)kRec * a.P * sel);
    for (int k = threadIdx.x; k < 4 * a.P; k += kTile) lds4[k] = src[k];
  }
  __syncthreads();
  const int npix = a.W * a.H;
  const int p0 = tile * kTile, pixel = p0 + threadIdx.x;
  const bool live = pixel < npix;
  float best = INFINITY;
  int id = -1;
  unsigned r8, g8, b8;
  {
    const float* sky = kPalette[kColSky];
    r8 = to_u8(sky[0]); g8 = to_u8(sky[1]); b8 = to_u8(sky[2]);
  }
  if (live) {
    // the camera: f = normalize(target - eye), r = normalize(f x z), u = r x f
    V3 anchor = v3(0, 0, 0);
    const int e = a.env_ids ? a.env_ids[sel] : sel;
    if (a.follow && e >= 0 && e < a.n_env) anchor = ld3(a.root + (size_t)13 * e * a.rows_per_env);
    const V3 eye = anchor + ld3(a.eye), tgt = anchor + ld3(a.tgt);
    V3 f = tgt - eye;
    f = f * (1.0f / sqrtf(dot(f, f)));
    V3 r = cross(f, v3(0, 0, 1));
    r = r * (1.0f / sqrtf(dot(r, r)));
    const V3 u = cross(r, f);
    const int i = pixel / a.W, j = pixel - i * a.W;
    const float px = (2.0f * ((float)j + 0.5f) / (float)a.W - 1.0f) * a.tan_half * (float)a.W / (float)a.H;
    const float py = (1.0f - 2.0f * ((float)i + 0.5f) / (float)a.H) * a.tan_half;
    V3 d = f + r * px + u * py;
    d = d * (1.0f / sqrtf(dot(d, d)));
    V3 nw = v3(0, 0, 1);
    int colour = 0;
    for (int p = 0; p < a.P; p++) {   // uniform: every lane of the wave is on primitive p
      const float* q = rec + kRec * p;
      const unsigned word = __float_as_uint(q[15]);
      const int type = (int)(word & 0xffu);
      if (type == kNone) continue;
      const V3 ow = eye - v3(q[9], q[10], q[11]);
      const V3 sz = v3(q[12], q[13], q[14]);
      if (type != MG_GT_PLANE) {
        // cull: a ray that passes the primitive's bounding sphere cannot hit it.  The bound is grown by 1 % of the
        // squared radius and by 1e-5 of the squared distance (fp32 rounding of |ow|^2 - (ow . d)^2 is below 1e-6 of
        // it), so no ray that touches the primitive is rejected; a wave whose rays all pass skips the primitive.
        const float rb2 = bound_radius2(type, sz);
        const float ww = dot(ow, ow), bd = dot(ow, d);
        if (ww - bd * bd > rb2 * 1.01f + 1e-5f * ww + 1e-9f) continue;
      }
      const V3 ol = v3(q[0] * ow.x + q[3] * ow.y + q[6] * ow.z, q[1] * ow.x + q[4] * ow.y + q[7] * ow.z,
                       q[2] * ow.x + q[5] * ow.y + q[8] * ow.z);
      const V3 dl = v3(q[0] * d.x + q[3] * d.y + q[6] * d.z, q[1] * d.x + q[4] * d.y + q[7] * d.z,
                       q[2] * d.x + q[5] * d.y + q[8] * d.z);
      V3 nl;
      const float t = hit_primitive(type, ol, dl, sz, a.m, &nl);
      if (t < best) {   // strict: a tie stays with the lower id
        best = t;
        id = p;
        colour = (int)(word >> 8);
        nw = v3(q[0] * nl.x + q[1] * nl.y + q[2] * nl.z, q[3] * nl.x + q[4] * nl.y + q[5] * nl.z,
                q[6] * nl.x + q[7] * nl.y + q[8] * nl.z);
      }
    }
    if (id >= 0) {
      if (colour == kColGround) {   // 1 m checker
        const V3 hp = eye + d * best;
        colour += ((int)floorf(hp.x) + (int)floorf(hp.y)) & 1;
      }
      const float il = 1.0f / sqrtf(0.3f * 0.3f + 0.2f * 0.2f + 1.0f);
      const float ndl = (nw.x * 0.3f + nw.y * 0.2f + nw.z) * il;
      const float sh = 0.35f + 0.65f * fmaxf(0.0f, ndl);
      const float* base = kPalette[colour];
      r8 = to_u8(base[0] * sh); g8 = to_u8(base[1] * sh); b8 = to_u8(base[2] * sh);
    }
    const size_t o = (size_t)npix * sel + pixel;
    if (a.depth) a.depth[o] = best;
    if (a.ids) a.ids[o] = id;
  }
  if (a.rgb) {   // uniform
    pix[3 * threadIdx.x + 0] = (unsigned char)r8;
    pix[3 * threadIdx.x + 1] = (unsigned char)g8;
    pix[3 * threadIdx.x + 2] = (unsigned char)b8;
    __syncthreads();
    const int nb = 3 * (npix - p0 < kTile ? npix - p0 : kTile);
    unsigned char* o = a.rgb + ((size_t)npix * sel + p0) * 3;
    for (int k = threadIdx.x; k < nb; k += kTile) o[k] = pix[k];
  }
}

}  // namespace mgrd
