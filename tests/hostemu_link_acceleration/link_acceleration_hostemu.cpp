// link_acceleration_hostemu.cpp - TEST-ONLY host build of the device routines behind mppi_sim_link_acceleration and
// mppi_sim_wrench_forces (csrc/mppi_device.hpp: link_accelerations, link_acceleration, gather_link_wrench, wrench_joint_forces): g++
// compiles the very templates that k_sim_link_acceleration and k_sim_wrench_forces instantiate per env, so their fp32 arithmetic meets
// the fp64 references on a machine without a GPU (tests/test_link_acceleration.py).  Nothing in the product path loads this library;
// the staged loads and stores of the kernels are exercised by tests/test_gpu_link_acceleration.py only.
#include <string>

#include "../../mppi-isaac_amd/csrc/mppi_pack.hpp"

using namespace mppi;

static_assert(kIdGravity == MPPI_ID_GRAVITY && kIdVelocity == MPPI_ID_VELOCITY, "inverse-dynamics term bits");

namespace {
// -1: the model does not pack, -2: a moving base, -3: a tree this build does not instantiate; 0: fn(T, m) ran
template <class F>
int with_tree(const mppi_model_t *model, F &&fn) {
    DevModel m;
    std::string err;
    if (!pack_model(*model, m, err)) return -1;
    if (m.floating || m.n_bases > 1) return -2;
    int parents[MPPI_MAX_BODIES];
    for (int i = 0; i < m.nb; i++) parents[i] = m.b[i].k0.parent;
    bool built = false;
    const bool ok = dispatch_topology(m.nb, parents, [&](auto topo) {
        using T = decltype(topo);
        if constexpr (T::NBASE == 1) {
            built = true;
            fn(topo, m);
        }
    });
    return ok && built ? 0 : -3;
}
template <class T>
void env_pose(DevModel &m, const float *root, const float *q, Pose<T> &P, V3 *d) {
    P.pb = loadv(root + 13 * m.robot_actor);
    P.Rb = quat_to_R(root + 13 * m.robot_actor + 3);
    forward_kinematics_offsets<T>(m, q, P, d);
}
}  // namespace

extern "C" {
// acc [K][rb_count][6] of rigid bodies rb_first .. of the packed model at (root, q [K][n], qd [K][n]) for qdd [K][n] (or null) and the
// bits in terms.  -1 .. -3: as with_tree, -4: bits other than MPPI_ID_VELOCITY in terms, -5: a null acc, -6: a range outside
// [0, n_rb) - nothing is written then
int emu_link_acceleration(const mppi_model_t *model, int K, const float *root, const float *q, const float *qd, int rb_first, int rb_count,
                          const float *qdd, int terms, float *acc) {
    if (!acc) return -5;
    if (rb_first < 0 || rb_count < 1 || rb_first >= model->n_rb || rb_count > model->n_rb - rb_first) return -6;
    if (terms & ~MPPI_ID_VELOCITY) return -4;
    return with_tree(model, [&](auto topo, DevModel &m) {
        using T = decltype(topo);
        constexpr int n = T::NB;
        for (int k = 0; k < K; k++) {
            Pose<T> P;
            V3 d[n ? n : 1];
            BodyMotion<T> B;
            env_pose<T>(m, root, q + (size_t)k * n, P, d);
            link_accelerations<T>(P, d, qd + (size_t)k * n, qdd ? qdd + (size_t)k * n : nullptr, terms, B);
            for (int j = 0; j < rb_count; j++) link_acceleration<T>(m, P, B, rb_first + j - m.robot_first_rb, acc + ((size_t)k * rb_count + j) * 6);
        }
    });
}
// tau [K][n] = sum_b J_b^T w[k][b] for the wrenches w [K][rb_count][6] on rigid bodies rb_first ..  -1 .. -3: as with_tree, -5: a null
// pointer, -6: a range outside [0, n_rb) - nothing is written then
int emu_wrench_forces(const mppi_model_t *model, int K, const float *root, const float *q, int rb_first, int rb_count, const float *w, float *tau) {
    if (!w || !tau) return -5;
    if (rb_first < 0 || rb_count < 1 || rb_first >= model->n_rb || rb_count > model->n_rb - rb_first) return -6;
    return with_tree(model, [&](auto topo, DevModel &m) {
        using T = decltype(topo);
        constexpr int n = T::NB;
        for (int k = 0; k < K; k++) {
            Pose<T> P;
            V3 d[n ? n : 1], F[n ? n : 1], N[n ? n : 1];
            env_pose<T>(m, root, q + (size_t)k * n, P, d);
            for (int i = 0; i < n; i++) F[i] = N[i] = V3{0.f, 0.f, 0.f};
            for (int j = 0; j < rb_count; j++) {
                const float *r = w + ((size_t)k * rb_count + j) * 6;
                gather_link_wrench<T>(m, P, rb_first + j - m.robot_first_rb, V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, F, N);
            }
            wrench_joint_forces<T>(P, d, F, N, tau + (size_t)k * n);
        }
    });
}
}
