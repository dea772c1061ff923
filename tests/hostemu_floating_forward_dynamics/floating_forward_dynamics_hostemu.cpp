// floating_forward_dynamics_hostemu.cpp - TEST-ONLY host build of floating_forward_dynamics (csrc/mppi_device.hpp): g++ compiles the
// very template that k_sim_floating_forward_dynamics instantiates per env, so its fp32 arithmetic meets the fp64 reference on a
// machine without a GPU (tests/test_floating_forward_dynamics.py).  Nothing in the product path loads this library; the staged
// load and store of the kernel are exercised by tests/test_gpu_floating_forward_dynamics.py only.
#include <string>

#include "../../mppi-isaac_amd/csrc/mppi_pack.hpp"

using namespace mppi;

static_assert(kIdGravity == MPPI_ID_GRAVITY && kIdVelocity == MPPI_ID_VELOCITY, "dynamics term bits");

extern "C" {
// vd [K][6 + n] of the packed model at (root [K][n_actors][13], q [K][n], qd [K][n]) for tau [K][6 + n] (or null) and the MPPI_ID_*
// bits in terms; every env takes its base pose and twist from its own root rows.  -1: the model does not pack, -2: a fixed base,
// -7: a forest of several moving bases, -3: a tree this build does not instantiate, -4: unknown bits in terms, -5: a null vd -
// nothing is written then
int emu_floating_forward_dynamics(const mppi_model_t *model, int K, const float *root, const float *q, const float *qd, const float *tau, int terms,
                                  float *vd) {
    if (!vd) return -5;
    if (terms & ~(MPPI_ID_GRAVITY | MPPI_ID_VELOCITY)) return -4;
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
            constexpr int n = T::NB, len = 6 + n;
            for (int k = 0; k < K; k++) {
                const float *row = root + ((size_t)k * m.n_actors + m.robot_actor) * 13;
                Pose<T> P;
                V3 d[n ? n : 1];
                P.pb = loadv(row);
                P.Rb = quat_to_R(row + 3);
                forward_kinematics_offsets<T>(m, q + (size_t)k * n, P, d);
                float v[len];
                for (int j = 0; j < 6; j++) v[j] = row[7 + j];
                for (int i = 0; i < n; i++) v[6 + i] = qd[(size_t)k * n + i];
                floating_forward_dynamics<T>(m, P, d, v, tau ? tau + (size_t)k * len : nullptr, terms, vd + (size_t)k * len);
            }
        }
    });
    return ok && built ? 0 : -3;
}
}
