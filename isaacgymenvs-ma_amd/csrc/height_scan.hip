// height_scan.hip — mg_height_scan's kernel, in a translation unit (and so a code object) of its own: build.py links
// it last, and the code objects before it are what they are without it.
#include "common.hpp"

namespace mgi {
// The terrain heights under a pattern of points that turns with each actor's yaw (the reference's get_heights,
// tasks/anymal_terrain.py:515-538).  One thread per (actor, point), consecutive threads on consecutive
// points of an actor: the stores to out (N, P) coalesce, the actor's root row and origin are the same address across
// most of a wave, the two table reads are gathers.  Both cell indices are clamped, so every read is inside the table.
static __global__ __launch_bounds__(256) void k_height_scan(const float* __restrict__ root_states,
                                                            const float* __restrict__ points, int P, mg_heightfield hf,
                                                            float* __restrict__ out, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long a = i / P;
  const int k = (int)(i - a * P);
  const float* r = root_states + 13 * a;
  // quat_apply_yaw: the quaternion's x and y zeroed, the rest normalised and applied to (px, py, 0)
  const float qz = r[5], qw = r[6];
  const float il = 1.0f / sqrtf(qz * qz + qw * qw);
  const float z = qz * il, w = qw * il;
  const float c = w * w - z * z, s = 2.0f * w * z;  // cosine and sine of the yaw
  const float px = points[2 * k], py = points[2 * k + 1];
  float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  if (hf.env_origins) {
    ox = hf.env_origins[3 * a];
    oy = hf.env_origins[3 * a + 1];
    oz = hf.env_origins[3 * a + 2];
  }
  const float X = (c * px - s * py) + r[0] + ox, Y = (s * px + c * py) + r[1] + oy;
  // trunc, then the clip (a NaN or a value past the int range converts to a value the clip brings inside)
  int ix = (int)((X - hf.x0) / hf.dx), iy = (int)((Y - hf.y0) / hf.dx);
  ix = ix < 0 ? 0 : (ix > hf.nx - 2 ? hf.nx - 2 : ix);
  iy = iy < 0 ? 0 : (iy > hf.ny - 2 ? hf.ny - 2 : iy);
  const float* h = hf.heights + (size_t)ix * hf.ny + iy;
  out[i] = fminf(h[0], h[hf.ny + 1]) - oz;
}

void launch_height_scan(hipStream_t s, const mg_sim* sim, const float* points, int P, float* out) {
  const long total = (long)sim->n * P;
  hipLaunchKernelGGL(k_height_scan, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     (const float*)sim->views.root_states, points, P, sim->hf, out, total);
}
}  // namespace mgi
