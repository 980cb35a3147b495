// Host driver of rmp2_forward_dynamics.h for tests/test_forward_dynamics_host.py: no GPU, the device routines' own code on the
// CPU, with the template sizes the library picks (N by the dof count, SLOTS by the program).  Input (argv[1], native byte order;
// tests/forward_dynamics_reference.py write_driver_input): int32 n_ops, n_frames, n_dof, n_slots, n_states, mode (0 mass matrix,
// 1 forward dynamics, 2 dynamics step), drive, substeps, has_limit; float dt; per op int32 frame, restore, save, jtype, qidx,
// uint32 anc_mask, float axis[3], Tc[12]; float inert[n_frames][10]; float base_acc[3] (-g); float limit[n_dof]; float q, qd,
// u [n_states][n_dof].  Output (argv[2]): mode 0: float M[n_states][n_dof][n_dof]; mode 1: float qdd[n_states][n_dof]; mode 2:
// float q, qd, qdd, tau [n_states][n_dof] each.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rmp2_forward_dynamics.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

struct Job {
  std::vector<rmp2::DevOp> ops;
  int n, B, mode, drive, substeps;
  float dt;
  std::vector<float> inert, acc, lim, q, qd, u, M, qdd, tau;
  bool has_lim;
};

template <int N, int SLOTS>
static void run(Job& j) {
  const int n = j.n;
  for (int b = 0; b < j.B; ++b) {
    const size_t o = (size_t)b * n;
    if (j.mode == 0)
      rmp2::mass_matrix_robot<N, SLOTS>(j.ops.data(), (int)j.ops.size(), n, j.inert.data(), j.q.data() + o, j.M.data() + o * n);
    else
      rmp2::dynamics_step_robot<N, SLOTS>(j.ops.data(), (int)j.ops.size(), n, j.inert.data(), j.acc.data(), j.q.data() + o,
                                          j.qd.data() + o, j.u.data() + o, j.mode == 2 && j.drive == RMP2_DRIVE_ACCEL,
                                          j.has_lim ? j.lim.data() : nullptr, j.dt, j.mode == 2 ? j.substeps : 1, j.mode == 2,
                                          j.qdd.data() + o, j.mode == 2 ? j.tau.data() + o : nullptr);
  }
}

template <int N>
static void run_n(int slots, Job& j) {
  if (slots == 0) run<N, 0>(j);
  else if (slots == 1) run<N, 1>(j);
  else run<N, 2>(j);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[9];
  Job j;
  if (!rd(f, hdr, 9) || !rd(f, &j.dt, 1)) return 4;
  const int n_ops = hdr[0], F = hdr[1], n = hdr[2], slots = hdr[3], B = hdr[4];
  j.n = n, j.B = B, j.mode = hdr[5], j.drive = hdr[6], j.substeps = hdr[7], j.has_lim = hdr[8] != 0;
  if (n_ops < 1 || n_ops > RMP2_MAX_FRAMES || F != n_ops || n < 1 || n > RMP2_MAX_DOF || slots < 0 || slots > 2 || B < 0 ||
      j.mode < 0 || j.mode > 2 || j.substeps < 1)
    return 5;
  j.ops.resize(n_ops);
  for (auto& op : j.ops) {
    std::memset(&op, 0, sizeof(op));
    int32_t v[5];
    uint32_t mask;
    if (!rd(f, v, 5) || !rd(f, &mask, 1) || !rd(f, op.axis, 3) || !rd(f, op.Tc, 12)) return 6;
    op.frame = v[0], op.restore = v[1], op.save = v[2], op.jtype = v[3], op.qidx = v[4], op.anc_mask = mask;
    if (op.frame < 0 || op.frame >= F || op.qidx >= n || op.restore >= slots || op.save >= slots) return 7;
  }
  j.inert.resize((size_t)F * rmp2::kInertialFloats), j.acc.resize(3), j.lim.resize(n);
  j.q.resize((size_t)B * n), j.qd.resize(j.q.size()), j.u.resize(j.q.size()), j.qdd.resize(j.q.size()), j.tau.resize(j.q.size());
  j.M.resize(j.mode == 0 ? j.q.size() * n : 0);
  if (!rd(f, j.inert.data(), j.inert.size()) || !rd(f, j.acc.data(), 3) || !rd(f, j.lim.data(), j.lim.size()) ||
      !rd(f, j.q.data(), j.q.size()) || !rd(f, j.qd.data(), j.qd.size()) || !rd(f, j.u.data(), j.u.size()))
    return 8;
  fclose(f);
  if (n <= 2) run_n<2>(slots, j);
  else if (n <= 9) run_n<9>(slots, j);
  else run_n<16>(slots, j);
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 9;
  if (j.mode == 0) fwrite(j.M.data(), sizeof(float), j.M.size(), g);
  if (j.mode == 2) {
    fwrite(j.q.data(), sizeof(float), j.q.size(), g);
    fwrite(j.qd.data(), sizeof(float), j.qd.size(), g);
  }
  if (j.mode != 0) fwrite(j.qdd.data(), sizeof(float), j.qdd.size(), g);
  if (j.mode == 2) fwrite(j.tau.data(), sizeof(float), j.tau.size(), g);
  return fclose(g) == 0 ? 0 : 10;
}
