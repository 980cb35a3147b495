// Host driver of the link-capsule closest-point closed forms of rmp2_device.h for tests/test_link_pairs_host.py: no GPU, the
// device routines' own code on the CPU (segment_segment, link_pair_fields, link_normal_length are __host__ __device__).
// Input (argv[1], native byte order): int32 n; per pair 15 floats: link axis A[3], B[3], link radius, primitive record
// ca = (a.xyz, radius), cb = (b.xyz, -).  Output (argv[2]) per pair 15 floats:
//   s, t                       segment_segment's parameters
//   p_link[3], normal[3], dist link_pair_fields with P3 = 0 (a distance leaf's fields)
//   p_link[3], p_obs[3]        the closest-point stage's form: X - r_link n / len, Y + r_obs n / len, len = link_normal_length(n)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "rmp2_device.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 4;
  std::vector<float> in((size_t)n * 15), out((size_t)n * 15);
  if (fread(in.data(), sizeof(float), in.size(), f) != in.size()) return 5;
  fclose(f);
  for (int i = 0; i < n; ++i) {
    const float* p = in.data() + (size_t)i * 15;
    float* o = out.data() + (size_t)i * 15;
    const float A[3] = {p[0], p[1], p[2]}, B[3] = {p[3], p[4], p[5]};
    const float lr = p[6];
    const float4 ca = make_float4(p[7], p[8], p[9], p[10]), cb = make_float4(p[11], p[12], p[13], p[14]);
    const float C[3] = {ca.x, ca.y, ca.z}, D[3] = {cb.x, cb.y, cb.z};
    float s, t;
    rmp2::segment_segment(A, B, C, D, s, t);
    o[0] = s, o[1] = t;
    const float LD[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const float laa = rmp2::dot3(LD, LD);
    const float inv_laa = laa > 0.f ? 1.0f / laa : 0.f;
    const float zero3[3] = {0.f, 0.f, 0.f};
    rmp2::link_pair_fields(A, LD, laa, inv_laa, lr, ca, cb, zero3, o + 2, o + 5, o[8]);
    float X[3], Y[3], nv[3];
    for (int c = 0; c < 3; ++c) {
      X[c] = A[c] + s * (B[c] - A[c]);
      Y[c] = C[c] + t * (D[c] - C[c]);
      nv[c] = X[c] - Y[c];
    }
    const float inv = 1.0f / rmp2::link_normal_length(nv);
    for (int c = 0; c < 3; ++c) {
      o[9 + c] = X[c] - lr * inv * nv[c];
      o[12 + c] = Y[c] + ca.w * inv * nv[c];
    }
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 6;
  fwrite(out.data(), sizeof(float), out.size(), g);
  return fclose(g) == 0 ? 0 : 7;
}
