// Host driver of rmp2_hull.h hull_pair_closest for tests/test_self_hulls_host.py: no GPU, the device routine's own code on the
// CPU.  Input (argv[1], native byte order): int32 n_hulls; per hull int32 nv, nf, float verts[nv][3], float planes[nf][4]; int32
// n_queries; per query int32 hull_a, hull_b, double Rm[9] (row-major), double t[3] -- B placed in A's coordinates by Rm y + t.
// Output (argv[2]): per query double pa[3], pb[3], u[3], gap, iters, face.
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
    int32_t ab[2];
    double Rm[9], t[3];
    if (!rd(f, ab, 2) || !rd(f, Rm, 9) || !rd(f, t, 3) || ab[0] < 0 || ab[0] >= nh || ab[1] < 0 || ab[1] >= nh) return 9;
    const std::vector<float4>&VA = V[ab[0]], &PA = P[ab[0]], &VB = V[ab[1]], &PB = P[ab[1]];
    const rmp2::PairHit hh = rmp2::hull_pair_closest(VA.data(), (int)VA.size(), PA.data(), (int)PA.size(), VB.data(), (int)VB.size(),
                                                     PB.data(), (int)PB.size(), Rm, t);
    const double out[12] = {hh.pa[0], hh.pa[1], hh.pa[2], hh.pb[0], hh.pb[1], hh.pb[2], hh.u[0],
                            hh.u[1],  hh.u[2],  hh.gap,   (double)hh.iters, (double)hh.face};
    fwrite(out, sizeof(double), 12, g);
  }
  fclose(f);
  return fclose(g) == 0 ? 0 : 10;
}
