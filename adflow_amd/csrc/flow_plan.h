// The kernel dispatch of one mean-flow (+ SA) evaluation as a value.  plan_flow() is the ONE place where scheme, level, flags and the
// kernel-selection tuning keys turn into kernels: the executors of api.hip (enqueue_turb_residual, enqueue_flow_fluxes, on
// the plain or the dual launchers; block_res_split_enqueue) launch what the plan names, and the Jacobian assembly reads from the same plan
// whether the marches write its snapshot.  Host only: no HIP types, no globals, no side effects.  The rules are those the executors
// held one by one; tests/test_dispatch_plan.py pins the launches they produce.
#pragma once
#include <cmath>

#include "internal.h"

struct FlowFacts {
    // of the KParams of the evaluation
    int spaceDiscr, viscous, fineGrid, fwMode, dissApprox, lumpedDiss, limiter, coarseInit, onlyRadii, doScaling;
    bool rvec;
    double rFil, adis;
    // of the call
    bool viscApprox;    // thin-layer viscous flux (ADFLOW_RES_VISC_APPROX; forward mode: and not viscPC)
    bool needGradHbm;   // the caller reads the nodal gradients from the block arrays (updateIntermed copy-out, blockette.F90:706-750)
    bool dual;          // forward mode: the kernels on dual numbers (kernels_ad.hip)
    bool wantFlow, wantTurb;
    // of the level
    bool atRest;        // no block with grid velocities / a rotational source: only the generic kernels carry them
    bool rans;
    // tuning keys
    int eulerMarch, inviscidMarch, roeMarch, viscousTiled, saMarch, pcFused, rvecJoint, jacSnap;
};

enum class InviscidK { None, EulerMarch, RoeMarch, FaceMarch, PcMarch, LevelGather };
enum class ViscousK { None, GfMarch, ThinLayerMarch, GatherExact, GatherApprox };
enum class TurbK { None, SaMarch, LevelGather };

struct FlowPlan {
    // EulerMarch: Euler + scalar JST, one k-marching launch over every block of the level (k_euler_march)
    // RoeMarch:   Roe upwind on the fine level, reconstruction once per cell (k_roe_march)
    // FaceMarch:  matrix dissipation / Roe upwind / scalar JST of NS + RANS over the tile table, every face once in k and i
    //             (k_inviscid_march); scalar JST with the entropy sensor is bound by memory like the gather form (1.06 vs 1.10 ms on
    //             8 x 128x128x96): only with tuning inviscid_march = 2
    // PcMarch:    first-order upwind + thin-layer viscous flux, both functions of the two cells of a face -- one march, dw written once
    //             (k_pc_march: it carries the viscous part, `viscous` is None)
    // LevelGather: the cell-gather kernel, one launch for every block of the level (blocks are independent given their halos)
    InviscidK inviscid;
    // GfMarch:        nodal gradients + face fluxes as ONE marching kernel (k_visc_gf): the gradients stay in LDS (and go to HBM only
    //                 when a caller reads them)
    // ThinLayerMarch: the thin-layer flux of the preconditioner assembly over the tile table (k_visc_approx_march; no gradients)
    // GatherExact / GatherApprox: the per-block gather kernels (viscousFlux / viscousFluxApprox)
    ViscousK viscous;
    TurbK turb;
    // viscous march first, inviscid march last: the inviscid kernel (Roe: bound by FP64 issue) adds the viscous sums it finds in
    // dw(2:5) instead of the viscous kernel reading dw back.  Any inviscid kernel over the tile table can take that role (Roe,
    // matrix dissipation, scalar JST of NS / RANS); not with the persistent fw of the Runge-Kutta stages.
    bool viscFirst;
    // what must exist before the kernels run
    bool needSensor;        // entropy sensor of the blocks whose state changed (plain scalar JST of NS / RANS)
    bool needFaceVectors;   // dI / dJ / dK of every block of the level in front of a viscous MARCH (the gather forms look per block)
    bool needTiles, needGfTiles;
    // timeStep_block: with matrix dissipation / Roe upwind nothing in the residual reads the spectral radii, and without updateIntermed
    // the reference's default path (blocketteResCore, blockette.F90:299-753) keeps them in the blockette's private arrays: they are not
    // an output of the evaluation.  Only scalar JST needs them (and the entropy sensor the same kernel leaves in ss).
    bool needTimeStep;
    // Euler + scalar JST: the marching kernel forms the radii itself when nothing else needs them (no updateIntermed: neither the radii
    // nor dtl are outputs, blockette.F90:660-750)
    bool radiiInMarch;
    // the matrix-free vector: the Roe march that follows the SA march in the same queue writes the turbulence entry with its own five
    // (tuning "rvec_joint", KParams::rvecTurbFromDw)
    bool roeWritesTurbRvec;
    // the wall stress reads the gradients of the node planes ON the wall faces only: when the flux kernel keeps its gradients in LDS
    // (k_visc_gf) those few nodes are formed again by the wall-stress launch instead of every node of the level being stored
    bool wallGradOnChip;
    // Jacobian assembly: the kernel that completes the mean-flow / turbulence residual writes the snapshot of the coloured evaluation
    // itself (KParams::snapTab, tuning "jac_snap")
    bool flowSnapInMarch, turbSnapInMarch;
};

inline FlowPlan plan_flow(const FlowFacts& f)
{
    FlowPlan p = {};
    const bool scalar = f.spaceDiscr == ADFLOW_DISS_SCALAR, upwind = f.spaceDiscr == ADFLOW_UPWIND;
    const bool diss = fabs(f.rFil) >= 1.e-10;
    const bool visc = f.viscous && diss;                 // a viscous flux is formed
    const bool tiled = f.viscousTiled >= 2;
    // (the approximate residual changes the Roe scheme only through the limiter: lumpedDiss = first order)
    const int lim = f.lumpedDiss ? ADFLOW_LIM_FIRST_ORDER : f.limiter;
    const bool roeTakes = f.roeMarch && upwind && f.fineGrid && roe_march_takes(lim);
    // the scheme of the preconditioner matrix that k_pc_march serves: first-order upwind (lumpedDiss, or the user's first-order limiter)
    // on the fine level, no matrix-free vector, no multigrid forcing
    const bool pcScheme = f.pcFused && upwind && f.fineGrid && lim == ADFLOW_LIM_FIRST_ORDER && !f.rvec && !f.coarseInit && roeTakes;
    // scalar JST: the marching form reads its sensor from b.ss -- the entropy sensor of NS / RANS, or the frozen sensor of the
    // approximate residual, which Euler has too
    const bool scalarMarch = f.inviscidMarch >= 2 && scalar && (f.viscous || f.dissApprox) && f.fineGrid;

    // ---- turbulence: blockResCore order, SA residual first (blockette.F90:806-851).  On a side queue beside the mean-flow kernels -- the
    // default of rounds 2-3 -- the march gains nothing since every march fills the device: 2.26 against 2.21 ms, round 4
    if (f.wantTurb && f.rans) {
        const bool march = f.dual ? (f.saMarch && f.pcFused)      // (moving blocks are refused by the forward-mode assembly)
                                  : (f.saMarch && f.atRest);
        p.turb = march ? TurbK::SaMarch : TurbK::LevelGather;
        p.turbSnapInMarch = f.jacSnap && march;
    }

    // ---- mean flow
    if (f.wantFlow && f.dual) {
        // forward mode: every march is gated by pc_fused; there is no Euler march (no dual form of the pipelined kernel)
        if (f.viscApprox && tiled && visc && pcScheme) {
            p.inviscid = InviscidK::PcMarch;
        } else {
            // (scalar JST only with the entropy sensor of NS / RANS on the fine level, as in the plain evaluation; the upwind scheme is
            // k_roe_march's or the gather kernel's: the dual per-face march has no upwind form)
            const bool faceTakes = f.inviscidMarch && !f.fwMode && !(f.dissApprox && !f.fineGrid) &&
                                   (scalar ? scalarMarch : f.spaceDiscr == ADFLOW_DISS_MATRIX);
            p.inviscid = (f.pcFused && roeTakes) ? InviscidK::RoeMarch : (f.pcFused && faceTakes) ? InviscidK::FaceMarch : InviscidK::LevelGather;
            const bool marched = p.inviscid != InviscidK::LevelGather;
            if (visc && !f.viscApprox) {
                // (k_visc_gf on dual numbers: 160 KB of LDS, one workgroup per CU -- fine level only, unlike the plain form)
                p.viscous = (f.pcFused && tiled && f.fineGrid) ? ViscousK::GfMarch : ViscousK::GatherExact;
                p.viscFirst = p.viscous == ViscousK::GfMarch && marched;
            } else if (visc) {
                // (the thin-layer march runs in front of the per-face march only: behind the dual Roe march the gather form follows)
                p.viscous = (tiled && f.fineGrid && p.inviscid == InviscidK::FaceMarch) ? ViscousK::ThinLayerMarch : ViscousK::GatherApprox;
                p.viscFirst = p.viscous == ViscousK::ThinLayerMarch;
            }
        }
        p.needFaceVectors = p.inviscid == InviscidK::PcMarch || p.viscous == ViscousK::GfMarch || p.viscous == ViscousK::ThinLayerMarch;
        // timeStep_block_d: only the scalar dissipation reads the spectral radii
        p.needTimeStep = scalar;
    } else if (f.wantFlow) {
        const bool eulerMarch = f.eulerMarch && !f.viscous && scalar && f.fineGrid && !f.dissApprox && f.atRest;
        // the approximate residual of the preconditioner matrix: the lumped scalar / matrix dissipation has a marching form on the fine
        // level (k_inviscid_march<.., APX>, round 6); the upwind scheme changes through its limiter only
        const bool approxOk = !f.dissApprox || upwind || (f.fineGrid && f.pcFused && !f.fwMode);
        const bool tileInviscid = f.inviscidMarch && (!scalar || scalarMarch) && approxOk && f.atRest;
        if (eulerMarch) {
            p.inviscid = InviscidK::EulerMarch;
            p.radiiInMarch = f.onlyRadii && diss && euler_march_radii_capable(f.fwMode, f.doScaling, f.adis);
        } else {
            p.needSensor = f.viscous && scalar && diss && !f.dissApprox;
            p.inviscid = !tileInviscid ? InviscidK::LevelGather : roeTakes ? InviscidK::RoeMarch : InviscidK::FaceMarch;
            if (visc && !f.viscApprox) {
                p.viscous = tiled ? ViscousK::GfMarch : ViscousK::GatherExact;
                p.viscFirst = tiled && !f.fwMode && tileInviscid && !f.dissApprox && !f.lumpedDiss;
            } else if (visc) {
                // thin-layer viscous flux of the preconditioner assembly: marching form over the tile table (blocks at rest, 4-row
                // tiles), in front of the inviscid march in the same order as the exact one
                p.viscous = (tiled && f.atRest) ? ViscousK::ThinLayerMarch : ViscousK::GatherApprox;
                p.viscFirst = tiled && !f.fwMode && tileInviscid;
                if (p.viscFirst && pcScheme) {
                    p.inviscid = InviscidK::PcMarch;
                    p.viscous = ViscousK::None;
                    p.viscFirst = false;
                }
            }
        }
        p.needFaceVectors = visc && p.viscous != ViscousK::GatherExact && p.viscous != ViscousK::GatherApprox;
    }
    if (!f.dual) p.needTimeStep = !p.radiiInMarch && !(f.onlyRadii && !scalar);

    p.needTiles = p.inviscid == InviscidK::EulerMarch || p.inviscid == InviscidK::RoeMarch || p.inviscid == InviscidK::FaceMarch ||
                  p.inviscid == InviscidK::PcMarch || p.viscous == ViscousK::ThinLayerMarch;
    p.needGfTiles = p.viscous == ViscousK::GfMarch;
    p.wallGradOnChip = tiled && !f.needGradHbm;
    p.flowSnapInMarch = f.jacSnap && p.inviscid == InviscidK::PcMarch;
    // the exact viscous residual on the upwind scheme ends in k_roe_march<.., ADDV, RV> when a matrix-free vector is the target: that
    // kernel can write all six entries of a cell (every block holds six variables: checked by the executor)
    p.roeWritesTurbRvec = !f.dual && f.rvec && f.rvecJoint && p.turb == TurbK::SaMarch && p.viscous == ViscousK::GfMarch && p.viscFirst &&
                          p.inviscid == InviscidK::RoeMarch;
    return p;
}
