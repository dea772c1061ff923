// floating_jacobian_hostemu.cpp - TEST-ONLY host build of the device routines behind mppi_sim_floating_jacobian and
// mppi_sim_floating_mass_matrix (csrc/mppi_device.hpp: floating_link_jacobian, floating_mass_matrix): g++ compiles the very
// templates that k_sim_floating_jacobian and k_sim_floating_mass_matrix instantiate per env, so their fp32 arithmetic meets the
// fp64 references on a machine without a GPU (tests/test_floating_jacobian_mass.py).  Nothing in the product path loads this
// library; the staged stores of the kernels are exercised by tests/test_gpu_floating_jacobian_mass.py only.
#include <string>

#include "../../mppi-isaac_amd/csrc/mppi_pack.hpp"

using namespace mppi;

namespace {
// -1: the model does not pack, -2: a fixed base, -7: a forest of several moving bases, -3: a tree this build does not
// instantiate; 0: fn(T, m) ran
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
// every env has a root tensor of its own: root [K][n_actors][13]
template <class T>
void env_pose(DevModel &m, const float *root, const float *q, Pose<T> &P, V3 *d) {
    P.pb = loadv(root + 13 * m.robot_actor);
    P.Rb = quat_to_R(root + 13 * m.robot_actor + 3);
    forward_kinematics_offsets<T>(m, q, P, d);
}
}  // namespace

extern "C" {
// J [K][rb_count][6][6 + n] of rigid bodies rb_first .. of the packed model at (root [K][n_actors][13], q [K][n]).  -1 -2 -3 -7: as
// with_moving_tree, -5: a null J, -6: a range outside [0, n_rb) - nothing is written then
int emu_floating_jacobian(const mppi_model_t *model, int K, const float *root, const float *q, int rb_first, int rb_count, float *J) {
    if (!J) return -5;
    if (rb_first < 0 || rb_count < 1 || rb_first >= model->n_rb || rb_count > model->n_rb - rb_first) return -6;
    return with_moving_tree(model, [&](auto topo, DevModel &m) {
        using T = decltype(topo);
        constexpr int n = T::NB, len = 6 * (6 + n);
        for (int k = 0; k < K; k++) {
            Pose<T> P;
            V3 d[n ? n : 1];
            env_pose<T>(m, root + (size_t)k * 13 * m.n_actors, q + (size_t)k * n, P, d);
            for (int j = 0; j < rb_count; j++) floating_link_jacobian<T>(m, P, d, rb_first + j - m.robot_first_rb, J + ((size_t)k * rb_count + j) * len);
        }
    });
}
// M [K][6 + n][6 + n].  -1 -2 -3 -7: as with_moving_tree, -5: a null M - nothing is written then
int emu_floating_mass_matrix(const mppi_model_t *model, int K, const float *root, const float *q, float *M) {
    if (!M) return -5;
    return with_moving_tree(model, [&](auto topo, DevModel &m) {
        using T = decltype(topo);
        constexpr int n = T::NB, len = (6 + n) * (6 + n);
        for (int k = 0; k < K; k++) {
            Pose<T> P;
            V3 d[n ? n : 1];
            env_pose<T>(m, root + (size_t)k * 13 * m.n_actors, q + (size_t)k * n, P, d);
            floating_mass_matrix<T>(m, P, d, M + (size_t)k * len);
        }
    });
}
}
