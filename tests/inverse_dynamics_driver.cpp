// Host driver of rmp2_dynamics.h inverse_dynamics_robot for tests/test_inverse_dynamics_host.py: no GPU, the device routine's own
// code on the CPU, with the template sizes the library picks (N by the dof count, SLOTS by the program).  Input (argv[1], native
// byte order; tests/dynamics_reference.py write_driver_input): int32 n_ops, n_frames, n_dof, n_slots, n_states; per op int32
// frame, restore, save, jtype, qidx, uint32 anc_mask, float axis[3], Tc[12]; float inert[n_frames][10]; float base_acc[3] (-g);
// float q, qd, qdd [n_states][n_dof].  Output (argv[2]): float tau[n_states][n_dof].
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rmp2_dynamics.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

template <int N, int SLOTS>
static void run(const std::vector<rmp2::DevOp>& ops, int n_dof, const float* inert, const float* acc, const float* q, const float* qd,
                const float* qdd, float* tau, int B) {
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * n_dof;
    rmp2::inverse_dynamics_robot<N, SLOTS>(ops.data(), (int)ops.size(), n_dof, inert, acc, q + o, qd + o, qdd + o, tau + o);
  }
}

template <int N>
static void run_n(int slots, const std::vector<rmp2::DevOp>& ops, int n_dof, const float* inert, const float* acc, const float* q,
                  const float* qd, const float* qdd, float* tau, int B) {
  if (slots == 0) run<N, 0>(ops, n_dof, inert, acc, q, qd, qdd, tau, B);
  else if (slots == 1) run<N, 1>(ops, n_dof, inert, acc, q, qd, qdd, tau, B);
  else run<N, 2>(ops, n_dof, inert, acc, q, qd, qdd, tau, B);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[5];
  if (!rd(f, hdr, 5)) return 4;
  const int n_ops = hdr[0], F = hdr[1], n = hdr[2], slots = hdr[3], B = hdr[4];
  if (n_ops < 1 || n_ops > RMP2_MAX_FRAMES || F != n_ops || n < 1 || n > RMP2_MAX_DOF || slots < 0 || slots > 2 || B < 0) return 5;
  std::vector<rmp2::DevOp> ops(n_ops);
  for (auto& op : ops) {
    std::memset(&op, 0, sizeof(op));
    int32_t v[5];
    uint32_t mask;
    if (!rd(f, v, 5) || !rd(f, &mask, 1) || !rd(f, op.axis, 3) || !rd(f, op.Tc, 12)) return 6;
    op.frame = v[0], op.restore = v[1], op.save = v[2], op.jtype = v[3], op.qidx = v[4], op.anc_mask = mask;
    if (op.frame < 0 || op.frame >= F || op.qidx >= n || op.restore >= slots || op.save >= slots) return 7;
  }
  std::vector<float> inert((size_t)F * rmp2::kInertialFloats), acc(3), q((size_t)B * n), qd(q.size()), qdd(q.size()), tau(q.size());
  if (!rd(f, inert.data(), inert.size()) || !rd(f, acc.data(), 3) || !rd(f, q.data(), q.size()) || !rd(f, qd.data(), qd.size()) ||
      !rd(f, qdd.data(), qdd.size()))
    return 8;
  fclose(f);
  if (n <= 2) run_n<2>(slots, ops, n, inert.data(), acc.data(), q.data(), qd.data(), qdd.data(), tau.data(), B);
  else if (n <= 9) run_n<9>(slots, ops, n, inert.data(), acc.data(), q.data(), qd.data(), qdd.data(), tau.data(), B);
  else run_n<16>(slots, ops, n, inert.data(), acc.data(), q.data(), qd.data(), qdd.data(), tau.data(), B);
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 9;
  fwrite(tau.data(), sizeof(float), tau.size(), g);
  return fclose(g) == 0 ? 0 : 10;
}
