// centroidal_hostemu.cpp - TEST-ONLY host build of momentum / floating_momentum and centroidal_matrix / floating_centroidal_matrix
// (csrc/mppi_device.hpp): g++ compiles the very templates that k_sim_momentum, k_sim_centroidal_matrix and
// k_sim_floating_centroidal_matrix instantiate per env, so their fp32 arithmetic meets the fp64 reference on a machine without a
// GPU (tests/test_centroidal.py).  Nothing in the product path loads this library; the staged stores of the kernels are exercised
// by tests/test_gpu_centroidal.py only.
#include <string>

#include "../../mppi-isaac_amd/csrc/mppi_pack.hpp"

using namespace mppi;

static_assert(kMomentumFloats == MPPI_MOMENTUM_FLOATS, "floats per row of mppi_sim_momentum");

namespace {
// f(topo, P, d, k) for every env of the packed model m at (root [K][n_actors][13], q [K][n]); false: a tree this build does not instantiate
template <class F>
bool for_each_env(DevModel &m, int K, const float *root, const float *q, F f) {
    int parents[MPPI_MAX_BODIES];
    for (int i = 0; i < m.nb; i++) parents[i] = m.b[i].k0.parent;
    bool built = false;
    const bool ok = dispatch_topology(m.nb, parents, [&](auto topo) {
        using T = decltype(topo);
        if constexpr (T::NBASE == 1) {
            built = true;
            for (int k = 0; k < K; k++) {
                const float *row = root + ((size_t)k * m.n_actors + m.robot_actor) * 13;
                Pose<T> P;
                V3 d[T::NB ? T::NB : 1];
                P.pb = loadv(row);
                P.Rb = quat_to_R(row + 3);
                forward_kinematics_offsets<T>(m, q + (size_t)k * T::NB, P, d);
                f(topo, P, d, k, row);
            }
        }
    });
    return ok && built;
}
}  // namespace

extern "C" {
// out [K][12] of the packed model at (root [K][n_actors][13], q [K][n], qd [K][n]); a moving base takes its pose and twist from every
// env's own root row.  -1: the model does not pack, -7: a forest of several moving bases, -3: a tree this build does not
// instantiate, -5: a null output - nothing is written then
int emu_momentum(const mppi_model_t *model, int K, const float *root, const float *q, const float *qd, float *out) {
    if (!out) return -5;
    DevModel m;
    std::string err;
    if (!pack_model(*model, m, err)) return -1;
    if (m.n_bases > 1) return -7;
    const bool ok = for_each_env(m, K, root, q, [&](auto topo, auto &P, const V3 *d, int k, const float *row) {
        using T = decltype(topo);
        constexpr int n = T::NB;
        float v[6 + n];
        for (int j = 0; j < 6; j++) v[j] = row[7 + j];
        for (int i = 0; i < n; i++) v[6 + i] = qd[(size_t)k * n + i];
        if (m.floating) floating_momentum<T>(m, P, d, v, out + (size_t)k * kMomentumFloats);
        else momentum<T>(m, P, d, v + 6, out + (size_t)k * kMomentumFloats);
    });
    return ok ? 0 : -3;
}
// A [K][6][n] (moving == 0) or [K][6][6 + n] (moving != 0).  -2: the wrong kind of base for the entry asked for, the other codes as above
int emu_centroidal_matrix(const mppi_model_t *model, int moving, int K, const float *root, const float *q, float *A) {
    if (!A) return -5;
    DevModel m;
    std::string err;
    if (!pack_model(*model, m, err)) return -1;
    if (m.n_bases > 1) return -7;
    if ((m.floating != 0) != (moving != 0)) return -2;
    const bool ok = for_each_env(m, K, root, q, [&](auto topo, auto &P, const V3 *d, int k, const float *) {
        using T = decltype(topo);
        constexpr int n = T::NB;
        if (moving) floating_centroidal_matrix<T>(m, P, d, A + (size_t)k * 6 * (6 + n));
        else centroidal_matrix<T>(m, P, d, A + (size_t)k * 6 * n);
    });
    return ok ? 0 : -3;
}
}
