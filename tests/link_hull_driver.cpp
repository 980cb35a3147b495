// Host driver of rmp2_hull.h hull_closest for tests/test_link_hulls_host.py: no GPU, the device routine's own code on the CPU.
// Input (argv[1], native byte order): int32 n_hulls; per hull int32 nv, nf, float verts[nv][3], float planes[nf][4]; int32
// n_queries; per query int32 hull, double a[3], b[3], r -- the axis a-b (a == b: a sphere) of radius r in the hull's coordinates.
// Output (argv[2]): per query double hp[3], xp[3], u[3], gap, iters.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "rmp2_hull.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t nh = 0;
  if (!rd(f, &nh, 1) || nh < 1) return 4;
  std::vector<std::vector<float4>> V(nh), P(nh);
  for (int h = 0; h < nh; ++h) {
    int32_t nv = 0, nf = 0;
    if (!rd(f, &nv, 1) || !rd(f, &nf, 1) || nv < 1 || nf < 1) return 5;
    std::vector<float> v(3 * (size_t)nv), p(4 * (size_t)nf);
    if (!rd(f, v.data(), v.size()) || !rd(f, p.data(), p.size())) return 6;
    for (int i = 0; i < nv; ++i) V[h].push_back(make_float4(v[3 * i], v[3 * i + 1], v[3 * i + 2], 0.f));
    for (int i = 0; i < nf; ++i) P[h].push_back(make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]));
  }
  int32_t nq = 0;
  if (!rd(f, &nq, 1) || nq < 0) return 7;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 8;
  for (int k = 0; k < nq; ++k) {
    int32_t h;
    double abr[7];
    if (!rd(f, &h, 1) || !rd(f, abr, 7) || h < 0 || h >= nh) return 9;
    const rmp2::HullHit hh = rmp2::hull_closest(V[h].data(), (int)V[h].size(), P[h].data(), (int)P[h].size(), abr, abr + 3, abr[6]);
    const double out[11] = {hh.hp[0], hh.hp[1], hh.hp[2], hh.xp[0], hh.xp[1], hh.xp[2], hh.u[0], hh.u[1], hh.u[2], hh.gap, (double)hh.iters};
    fwrite(out, sizeof(double), 11, g);
  }
  fclose(f);
  return fclose(g) == 0 ? 0 : 10;
}
