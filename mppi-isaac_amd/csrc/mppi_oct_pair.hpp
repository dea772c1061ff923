// mppi_oct_pair.hpp - the contact-free octet rollout with HELPER WAVEFRONTS: a workgroup of two owner wavefronts (the octet
// layout of mppi_oct.hpp, eight samples each) and two helper wavefronts in the same lane layout, helper w serving owner w lane
// for lane.
//
// Why: the octet kernel is bound by the instruction count of a lone wavefront per SIMD, and the other SIMDs of its CU idle.  Of a
// horizon step only the articulated-body substeps feed the next step; forming the controls (noise loads, clamps, du stores, control
// cost), the pose of the cost link, the stage cost and the visualisation row feed nothing back.  They move to the helper.
//
// One-directional traffic through LDS, one workgroup barrier per horizon step:
//   control table   u[t][sample 0..15][stride]   written by the helpers (row t + 2 while the owners compute step t), read by the
//                                                 owners (the targets of step t: 16-byte reads) and by the record's row sums
//   hand-over ring  two slots of one 16-byte word per owner lane (A: the world pose of the body that carries the cost link after
//                   the uniform select - R columns 0, 1, 2 and p - or (q0, q1) for the point-robot cost; B: the same for the
//                   visualised link when it is another one).  The owner writes slot t & 1 and arrives at barrier 11; the helper
//                   reads it between barrier 11 of step t and of step t + 1, the owner writes it again only behind the latter.
// Barrier ids (MPPI_BARRIER: phase canaries in the check build): 10 - row 0 of the table is written; 11 - step t is handed over
// and rows <= t + 1 of the table are written.  Every wavefront of the workgroup executes every barrier: wavefronts whose samples
// do not exist compute the last existing sample again (same values to the same addresses) and keep their results to themselves.
#pragma once
#include "mppi_oct.hpp"
#include "mppi_quad.hpp"

namespace mppi {

#if defined(__HIP_DEVICE_COMPILE__)
constexpr int kPairMaxH = 32;  // rows of the control table (longer horizons keep the kernel without helpers)
template <class T>
struct PairLayout {
    static constexpr int MAXC = T::NB < kMaxNu ? T::NB : kMaxNu;
    static constexpr int kStride = (MAXC + 3) & ~3;        // floats per (step, sample): whole 16-byte words
    static constexpr int kRow = 16 * kStride;              // floats per step
    static constexpr int kTable = kPairMaxH * kRow;
};
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef MPPI_LDS_AS f32x4 LF4;

// OWNER: the state and the dynamics of the sample, nothing else.  `urow`: the sample's entry of row 0 of the control table,
// `xa` / `xb`: this lane's word of slot 0 of the hand-over ring (slot 1 lies `xslot` words further).
template <class T, int JT, class M, class AB>
__device__ __forceinline__ void pair_owner(M &m0, CCfg &cfg0, CCost &cost0, const float *dof0, const float *root, const MPPI_LDS_AS float *urow, LF4 *xa,
                                           LF4 *xb, int xslot, bool want_viz, const AB &ab) {
    constexpr int NB = T::NB, MAXC = PairLayout<T>::MAXC, kStride = PairLayout<T>::kStride, kRow = PairLayout<T>::kRow;
    // read once, kept in SGPRs across the horizon
    const int H = cfg0.H, kind = cost0.kind, link = cost0.link[0], viz_link = cfg0.viz_link;
    const bool cmd_identity = m0.cmd_identity != 0, need_link = kind == kCostPandaReach, point = kind == kCostPointReach;
    const bool own_viz = want_viz && (viz_link != link || !need_link);
    // the bodies that carry the cost link and the visualised link: resolved here, the steps keep the uniform select of the pose
    const int link_body = need_link ? quad_link_body<T>(m0, link) : -1, viz_body = own_viz ? quad_link_body<T>(m0, viz_link) : -1;
    constexpr bool JV = AB::kJointVectors;     // (mppi_oct.hpp OctAbaJv: joint 4v + r in lane r of register v)
    constexpr int NS = JV ? (NB + 3) / 4 : NB;
    static_assert(!JV || (NS * 4 <= kStride && NB == MAXC), "joint vectors: the table row holds a word per lane of every vector");
    QF q[NS], qd[NS], target[NS];
    if constexpr (JV) {
        ab.load_state(dof0, q, qd);
    } else {
        static_for<0, NB>([&](auto ic) MPPI_LAMBDA {
            constexpr int i = ic;
            q[i] = qrep(dof0[2 * i]);
            qd[i] = qrep(dof0[2 * i + 1]);
        });
    }
    QPose<T, JT> P;  // forward kinematics of the current q, carried across the whole horizon
    quad_base<T>(m0, root, P);
    if constexpr (JV) ab.template fk<T>(m0, q, P);
    else quad_fk<T>(m0, q, P);
    M *mp = &m0;
    MPPI_BARRIER(10);
    for (int t = 0; t < H; t++) {
        float u[kMaxNu];
#pragma unroll
        for (int c = MAXC; c < kMaxNu; c++) u[c] = 0.f;
        if (!JV || !cmd_identity) {
#pragma unroll
            for (int j = 0; j < kStride / 4; j++) {
                const f32x4 v = *reinterpret_cast<const LF4 *>(urow + t * kRow + 4 * j);
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (4 * j + c < MAXC) u[4 * j + c] = v[c];
            }
        }
        if constexpr (JV) {
            // joint vectors: this lane's joint's entry of the row, one 4-byte read per vector (the helpers write zeros beyond nu)
            if (cmd_identity) {
#pragma unroll
                for (int v = 0; v < NS; v++) target[v] = urow[t * kRow + 4 * v + ab.r];
            } else {
                ab.template targets_mapped<MAXC>(*launder(mp), u, target);
            }
        } else if (cmd_identity) {  // fixed-base arms, the point robot: one unit-gain command per body
            static_for<0, NB>([&](auto ic) MPPI_LAMBDA { target[ic] = qrep(u[ic < kMaxNu ? (int)ic : 0]); });
        } else {
            M &m = *launder(mp);
            static_for<0, NB>([&](auto ic) MPPI_LAMBDA {
                constexpr int i = ic;
                const CmdBlock b = load_block<CmdBlock>(m.b[i].cmd);
                float tg = 0.f;
#pragma unroll
                for (int c = 0; c < MAXC; c++) tg += b.v[c] * u[c];
                target[i] = qrep(tg);
            });
        }
        quad_step<T>(*mp, P, q, qd, target, ab);
        const int s = (t & 1) * xslot;
        if (need_link) {
            QM3 Rb;
            QF pb;
            quad_link_body_pose_at<T>(P, link_body, Rb, pb);
            xa[s] = f32x4{Rb.c[0], Rb.c[1], Rb.c[2], pb};
        } else if (point) {
            if constexpr (JV) xa[s] = f32x4{ab.template joint<0>(q), ab.template joint<(NB > 1 ? 1 : 0)>(q), 0.f, 0.f};
            else xa[s] = f32x4{q[0], q[NB > 1 ? 1 : 0], 0.f, 0.f};
        }
        if (own_viz) {
            QM3 Rb;
            QF pb;
            quad_link_body_pose_at<T>(P, viz_body, Rb, pb);
            xb[s] = f32x4{Rb.c[0], Rb.c[1], Rb.c[2], pb};
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the hand-over is in LDS before this wavefront arrives
        MPPI_BARRIER(11);
    }
}

// HELPER: controls, stage cost, discounted sum and visualisation of the owner's samples, lane for lane what quad_rollout does
// with them (the same functions on the same values in the same order: S comes out bit for bit).  Returns S + ctrl.
template <class T, class M>
__device__ __forceinline__ QF pair_helper(M &m0, CCfg &cfg0, CCost &cost0, LStep &sc, const float *eps, const float *prior, float *du, float *viz, int k,
                                          int row, MPPI_LDS_AS float *urow, const LF4 *xa, const LF4 *xb, int xslot) {
    constexpr int MAXC = PairLayout<T>::MAXC, kStride = PairLayout<T>::kStride, kRow = PairLayout<T>::kRow;
    const int K = cfg0.K, nu = cfg0.nu, H = cfg0.H, kind = cost0.kind, link = cost0.link[0], viz_link = cfg0.viz_link;
    const float lambda = cfg0.lambda, gamma = cfg0.gamma;
    const bool abs_cost = cfg0.noise_abs_cost != 0, want_viz = cfg0.want_rollouts && viz != nullptr;
    const bool need_link = kind == kCostPandaReach;
    const bool own_viz = want_viz && (viz_link != link || !need_link);
    const int g = cfg0.k_offset + k;
    const bool is_null = cfg0.sample_null_action && g == cfg0.k_total - 1;
    const bool is_prior = cfg0.use_priors && prior != nullptr && g == cfg0.k_total - 2;
    ControlRows<MAXC> rows;
    load_controls_q<MAXC>(sc, eps, prior, nu, K, 0, k, rows);
    const bool special_here = __builtin_amdgcn_ballot_w64(is_null || is_prior) != 0;  // wave-uniform
    const bool plain_controls = !special_here && nu == MAXC && !abs_cost;
    float ctrl = 0.f, disc = 1.f;
    QF S = qrep(0.f);
    // row t of the table (and the du row, and the control cost of step t); the noise of row t + 1 is requested behind it
    auto controls = [&](int t) MPPI_LAMBDA {
        float u[kMaxNu];
        ctrl += plain_controls ? apply_controls_q<MAXC, true>(sc, lambda, abs_cost, nu, K, rows, t, k, is_null, is_prior, false, du, u)
                               : apply_controls_q<MAXC, false>(sc, lambda, abs_cost, nu, K, rows, t, k, is_null, is_prior, false, du, u);
#pragma unroll
        for (int j = 0; j < kStride / 4; j++) {
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = 4 * j + c < MAXC ? u[4 * j + c] : 0.f;
            *reinterpret_cast<LF4 *>(urow + t * kRow + 4 * j) = v;
        }
        load_controls_q<MAXC>(sc, eps, prior, nu, K, t + 1 < H ? t + 1 : t, k, rows);
    };
    controls(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    MPPI_BARRIER(10);
    if (H > 1) controls(1);
    M *mp = &m0;
    for (int t = 0; t < H; t++) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the table rows written so far are in LDS
        MPPI_BARRIER(11);
        if (t + 2 < H) controls(t + 2);
        const int s = (t & 1) * xslot;
        QM3 Rl;  // pose of the cost link, shared with the rollout visualisation when that shows the same link
        QF pl = qrep(0.f);
        for (int c = 0; c < 3; c++) Rl.c[c] = qrep(0.f);
        QF q[2] = {qrep(0.f), qrep(0.f)};
        if (need_link) {
            const f32x4 a = xa[s];
            quad_link_from_body(launder(mp)->l[link], QM3{{a[0], a[1], a[2]}}, a[3], Rl, pl);
        } else if (kind == kCostPointReach) {
            const f32x4 a = xa[s];
            q[0] = a[0];
            q[1] = a[1];
        }
        S += disc * quad_stage_cost<T>(kind, sc, q, Rl, pl);
        disc *= gamma;
        if (want_viz) {
            QM3 R;
            QF p = pl;
            if (own_viz) {
                const f32x4 b = xb[s];
                quad_link_from_body(launder(mp)->l[viz_link], QM3{{b[0], b[1], b[2]}}, b[3], R, p);
            }
            viz[((unsigned)(t * 3 + row)) * (unsigned)K + (unsigned)k] = p;  // lane r stores component r (lane 3 mirrors lane 0)
        }
    }
    return S + ctrl;
}
#endif

}  // namespace mppi
