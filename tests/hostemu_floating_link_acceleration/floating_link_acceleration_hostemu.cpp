// floating_link_acceleration_hostemu.cpp - TEST-ONLY host build of the device routines behind mppi_sim_floating_link_acceleration and
// mppi_sim_floating_wrench_forces (csrc/mppi_device.hpp: floating_link_accelerations, floating_link_acceleration,
// gather_floating_link_wrench, floating_wrench_joint_forces): g++ compiles the very templates that k_sim_floating_link_acceleration and
// k_sim_floating_wrench_forces instantiate per env, so their fp32 arithmetic meets the fp64 references on a machine without a GPU
// (tests/test_floating_link_acceleration.py).  Nothing in the product path loads this library; the staged loads and stores of the
// kernels are exercised by tests/test_gpu_floating_link_acceleration.py only.
#include <string>

#include "../../mppi-isaac_amd/csrc/mppi_pack.hpp"

using namespace mppi;

static_assert(kIdGravity == MPPI_ID_GRAVITY && kIdVelocity == MPPI_ID_VELOCITY, "dynamics term bits");

namespace {
// -1: the model does not pack, -7: a forest of several moving bases, -2: a fixed base, -3: a tree this build does not instantiate;
// 0: fn(T, m) ran
template <class F>
int with_moving_tree(const mppi_model_t *model, F &&fn) {
    DevModel m;
    std::string err;
    if (!pack_model(*model, m, err)) return -1;
    if (m.n_bases > 1) return -7;
    if (!m.floating) return -2;
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
// the env's own base pose from its root rows (root [K][n_actors][13]) -> the robot's row
template <class T>
const float *env_pose(DevModel &m, const float *root, int k, const float *q, Pose<T> &P, V3 *d) {
    const float *row = root + ((size_t)k * m.n_actors + m.robot_actor) * 13;
    P.pb = loadv(row);
    P.Rb = quat_to_R(row + 3);
    forward_kinematics_offsets<T>(m, q, P, d);
    return row;
}
}  // namespace

extern "C" {
// acc [K][rb_count][6] of rigid bodies rb_first .. of the packed model at (root [K][n_actors][13], q [K][n], qd [K][n]) for vd [K][6 + n]
// (or null) and the bits in terms; every env takes its base pose and twist from its own root rows.  -1, -7, -2, -3: as
// with_moving_tree, -4: bits other than MPPI_ID_VELOCITY in terms, -5: a null acc, -6: a range outside [0, n_rb) - nothing is written then
int emu_floating_link_acceleration(const mppi_model_t *model, int K, const float *root, const float *q, const float *qd, int rb_first,
                                   int rb_count, const float *vd, int terms, float *acc) {
    if (!acc) return -5;
    if (rb_first < 0 || rb_count < 1 || rb_first >= model->n_rb || rb_count > model->n_rb - rb_first) return -6;
    if (terms & ~MPPI_ID_VELOCITY) return -4;
    return with_moving_tree(model, [&](auto topo, DevModel &m) {
        using T = decltype(topo);
        constexpr int n = T::NB, len = 6 + n;
        for (int k = 0; k < K; k++) {
            Pose<T> P;
            V3 d[n ? n : 1];
            BodyMotion<T> B;
            BaseMotion Bb;
            const float *row = env_pose<T>(m, root, k, q + (size_t)k * n, P, d);
            float v[len];
            for (int j = 0; j < 6; j++) v[j] = row[7 + j];
            for (int i = 0; i < n; i++) v[6 + i] = qd[(size_t)k * n + i];
            floating_link_accelerations<T>(P, d, v, vd ? vd + (size_t)k * len : nullptr, terms, B, Bb);
            for (int j = 0; j < rb_count; j++)
                floating_link_acceleration<T>(m, P, B, Bb, rb_first + j - m.robot_first_rb, acc + ((size_t)k * rb_count + j) * 6);
        }
    });
}
// tau [K][6 + n] = sum_b J_b^T w[k][b] for the wrenches w [K][rb_count][6] on rigid bodies rb_first ..  -1, -7, -2, -3: as
// with_moving_tree, -5: a null pointer, -6: a range outside [0, n_rb) - nothing is written then
int emu_floating_wrench_forces(const mppi_model_t *model, int K, const float *root, const float *q, int rb_first, int rb_count, const float *w,
                               float *tau) {
    if (!w || !tau) return -5;
    if (rb_first < 0 || rb_count < 1 || rb_first >= model->n_rb || rb_count > model->n_rb - rb_first) return -6;
    return with_moving_tree(model, [&](auto topo, DevModel &m) {
        using T = decltype(topo);
        constexpr int n = T::NB, len = 6 + n;
        for (int k = 0; k < K; k++) {
            Pose<T> P;
            V3 d[n ? n : 1], F[n ? n : 1], N[n ? n : 1];
            V3 Fb = {0.f, 0.f, 0.f}, Nb = Fb;
            env_pose<T>(m, root, k, q + (size_t)k * n, P, d);
            for (int i = 0; i < n; i++) F[i] = N[i] = V3{0.f, 0.f, 0.f};
            for (int j = 0; j < rb_count; j++) {
                const float *r = w + ((size_t)k * rb_count + j) * 6;
                gather_floating_link_wrench<T>(m, P, rb_first + j - m.robot_first_rb, V3{r[0], r[1], r[2]}, V3{r[3], r[4], r[5]}, F, N, Fb, Nb);
            }
            floating_wrench_joint_forces<T>(P, d, F, N, Fb, Nb, tau + (size_t)k * len);
        }
    });
}
// J [K][rb_count][6][6 + n]: floating_link_jacobian of the same bodies at the same poses (the host build's own Jacobian, for the
// column-by-column and row-by-row comparisons).  Return codes as above.
int emu_floating_link_jacobian(const mppi_model_t *model, int K, const float *root, const float *q, int rb_first, int rb_count, float *J) {
    if (!J) return -5;
    if (rb_first < 0 || rb_count < 1 || rb_first >= model->n_rb || rb_count > model->n_rb - rb_first) return -6;
    return with_moving_tree(model, [&](auto topo, DevModel &m) {
        using T = decltype(topo);
        constexpr int n = T::NB, len = 6 * (6 + n);
        for (int k = 0; k < K; k++) {
            Pose<T> P;
            V3 d[n ? n : 1];
            env_pose<T>(m, root, k, q + (size_t)k * n, P, d);
            for (int j = 0; j < rb_count; j++) floating_link_jacobian<T>(m, P, d, rb_first + j - m.robot_first_rb, J + ((size_t)k * rb_count + j) * len);
        }
    });
}
}
