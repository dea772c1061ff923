// inverse_dynamics_hostemu.cpp - TEST-ONLY host build of inverse_dynamics (csrc/mppi_device.hpp): g++ compiles the very template
// that k_sim_inverse_dynamics instantiates per env, so its fp32 arithmetic meets the fp64 oracle on a machine without a GPU
// (tests/test_inverse_dynamics.py).  Nothing in the product path loads this library; the staged load and store of the kernel
// are exercised by tests/test_gpu_inverse_dynamics.py only.
#include <string>

#include "../../mppi-isaac_amd/csrc/mppi_pack.hpp"

using namespace mppi;

static_assert(kIdGravity == MPPI_ID_GRAVITY && kIdVelocity == MPPI_ID_VELOCITY, "inverse-dynamics term bits");

extern "C" {
// tau [n] of the packed model at (root, q, qd) for qdd [n] (or null) and the MPPI_ID_* bits in terms.  -1: the model does not pack,
// -2: a moving base, -3: a tree this build does not instantiate, -4: unknown bits in terms - nothing is written then
int emu_inverse_dynamics(const mppi_model_t *model, const float *root, const float *q, const float *qd, const float *qdd, int terms, float *tau) {
    DevModel m;
    std::string err;
    if (!pack_model(*model, m, err)) return -1;
    if (m.floating || m.n_bases > 1) return -2;
    if (terms & ~(MPPI_ID_GRAVITY | MPPI_ID_VELOCITY)) return -4;
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
            inverse_dynamics<T>(m, P, d, qd, qdd, terms, tau);
        }
    });
    return ok ? 0 : -3;
}
}
