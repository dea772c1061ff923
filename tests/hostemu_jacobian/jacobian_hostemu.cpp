// jacobian_hostemu.cpp - TEST-ONLY host build of link_jacobian / mass_matrix (csrc/mppi_device.hpp): g++ compiles the very
// templates that k_sim_jacobian / k_sim_mass_matrix instantiate per env, so their fp32 arithmetic meets the fp64 oracle on a
// machine without a GPU (tests/test_jacobian_mass.py).  Nothing in the product path loads this library; the staging and the
// stores of the kernels are exercised by tests/test_gpu_jacobian_mass.py only.
#include <string>

#include "../../mppi-isaac_amd/csrc/mppi_pack.hpp"

using namespace mppi;

namespace {
// f(topology, model, pose, offsets) for the packed model at (root, q); -1: the model does not pack, -2: a moving base, -3: a tree
// this build does not instantiate
template <class F>
int with_pose(const mppi_model_t *model, const float *root, const float *q, F &&f) {
    DevModel m;
    std::string err;
    if (!pack_model(*model, m, err)) return -1;
    if (m.floating || m.n_bases > 1) return -2;
    int parents[MPPI_MAX_BODIES];
    for (int i = 0; i < m.nb; i++) parents[i] = m.b[i].k0.parent;
    const bool ok = dispatch_topology(m.nb, parents, [&](auto topo) {
        using T = decltype(topo);
        if constexpr (T::NBASE == 1) {
            Pose<T> P;
            V3 d[T::NB ? T::NB : 1];
            P.pb = loadv(root + 13 * m.robot_actor);
            P.Rb = quat_to_R(root + 13 * m.robot_actor + 3);
            forward_kinematics_offsets<T>(m, q, P, d);
            f(topo, m, P, d);
        }
    });
    return ok ? 0 : -3;
}
}  // namespace

extern "C" {
// out [n_rb][6][n]
int emu_jacobian(const mppi_model_t *model, const float *root, const float *q, float *out) {
    return with_pose(model, root, q, [&](auto topo, const DevModel &m, const auto &P, const V3 *d) {
        using T = decltype(topo);
        for (int b = 0; b < m.n_rb; b++) link_jacobian<T>(m, P, d, b - m.robot_first_rb, out + (size_t)b * 6 * T::NB);
    });
}
// out [n][n]
int emu_mass_matrix(const mppi_model_t *model, const float *root, const float *q, float *out) {
    return with_pose(model, root, q, [&](auto topo, const DevModel &m, const auto &P, const V3 *d) {
        using T = decltype(topo);
        mass_matrix<T>(m, P, d, out);
    });
}
}
