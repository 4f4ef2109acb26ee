"""Host-side mirror of the reference's operator surface for the hot path.

Method names follow the reference's shell routines:
`timeStep`, `initres`, `residual`, `blocketteRes`, `RungeKuttaSmoother`,
`DADISmoother`, `whalo2`; each forwards to the C-ABI of include/adflow_gpu.h.
Blocks are addressed like `flowDoms(nn, level, sps)` (1-based).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import numpy as np

from . import capi
from .params import FlowParams


class Engine:
    def __init__(self, device: int = 0, _lib_path=None):
        self.lib = capi.load(_lib_path)
        self._chk(self.lib.adflow_gpu_init(device))
        self.blocks: Dict[Tuple[int, int, int], object] = {}
        self._descs = {}
        self.prm = None

    def _chk(self, rc):
        capi.check(rc, self.lib)

    # ---- lifetime ---------------------------------------------------------
    def close(self):
        if self.lib is not None:
            self.lib.adflow_gpu_finalize()
            self.lib = None

    def device_name(self) -> str:
        buf = ctypes.create_string_buffer(256)
        self._chk(self.lib.adflow_gpu_device_name(buf, 256))
        return buf.value.decode()

    # ---- data model -------------------------------------------------------
    def set_options(self, prm: FlowParams):
        self.prm = prm
        o = capi.opts_from_params(prm)
        self._chk(self.lib.adflow_gpu_set_options(ctypes.byref(o)))

    def register(self, blk, nn: int = 1, level: int = 1, sps: int = 1, upload: bool = True):
        """flowDoms(nn,level,sps) <- blk ; host arrays stay owned by `blk`."""
        a = blk.a
        ib, jb, kb, ie, je, ke = blk.ib, blk.jb, blk.kb, blk.ie, blk.je, blk.ke
        for name, shape in (("dw", (ib + 1, jb + 1, kb + 1, blk.nw)), ("fw", (ib + 1, jb + 1, kb + 1, 5)),
                            ("dtl", (ie, je, ke)), ("radI", (ie, je, ke)), ("radJ", (ie, je, ke)),
                            ("radK", (ie, je, ke))):
            if name not in a:
                a[name] = np.zeros(shape, order="F")
        d = capi.desc_from_block(blk)
        self._descs[(nn, level, sps)] = d
        self.blocks[(nn, level, sps)] = blk
        self._chk(self.lib.adflow_gpu_block_register(nn, level, sps, ctypes.byref(d)))
        if upload:
            self.upload_geometry(nn, level, sps)
            self.upload_state(nn, level, sps)

    def release(self, nn=1, level=1, sps=1):
        self._chk(self.lib.adflow_gpu_block_release(nn, level, sps))
        self.blocks.pop((nn, level, sps), None)
        self._descs.pop((nn, level, sps), None)

    def release_all(self):
        self._chk(self.lib.adflow_gpu_release_all())
        self.blocks.clear()
        self._descs.clear()

    def upload_geometry(self, nn=1, level=1, sps=1):
        self._chk(self.lib.adflow_gpu_upload_geometry(nn, level, sps))

    def upload_state(self, nn=1, level=1, sps=1):
        self._chk(self.lib.adflow_gpu_upload_state(nn, level, sps))

    def download_state(self, nn=1, level=1, sps=1):
        self._chk(self.lib.adflow_gpu_download_state(nn, level, sps))

    def download_residual(self, nn=1, level=1, sps=1):
        self._chk(self.lib.adflow_gpu_download_residual(nn, level, sps))
        return self.blocks[(nn, level, sps)]["dw"]

    def download_array(self, which: int, out: np.ndarray, nn=1, level=1, sps=1):
        assert out.flags["F_CONTIGUOUS"] and out.dtype == np.float64
        self._chk(self.lib.adflow_gpu_download_array(nn, level, sps, which, out.ctypes.data))
        return out

    def upload_array(self, which: int, src: np.ndarray, nn=1, level=1, sps=1):
        assert src.flags["F_CONTIGUOUS"] and src.dtype == np.float64
        self._chk(self.lib.adflow_gpu_upload_array(nn, level, sps, which, src.ctypes.data))

    # ---- the hot path (reference shell-routine names) -----------------------
    def timeStep(self, level=1, onlyRadii=False):
        self._chk(self.lib.adflow_gpu_time_step(level, int(onlyRadii)))

    def initres(self, level, varStart, varEnd):
        self._chk(self.lib.adflow_gpu_initres(level, varStart, varEnd))

    def residual(self, level=1, rkStage=0):
        self._chk(self.lib.adflow_gpu_residual(level, rkStage))

    def referenceShockSensor(self, level=1):
        self._chk(self.lib.adflow_gpu_reference_shock_sensor(level))

    def registerWallAssociation(self, surfNodeIndices: np.ndarray, uv: np.ndarray, nn=1, level=1, sps=1):
        """flowDoms%surfNodeIndices (4,nx,ny,nz) int32 / %uv (2,nx,ny,nz), Fortran order"""
        assert surfNodeIndices.dtype == np.int32 and surfNodeIndices.flags["F_CONTIGUOUS"] and uv.flags["F_CONTIGUOUS"]
        self._chk(self.lib.adflow_gpu_wall_distance_register(nn, level, sps, surfNodeIndices.ctypes.data, uv.ctypes.data))

    def updateWallDistancesQuickly(self, xSurf: np.ndarray, level=1):
        xSurf = np.ascontiguousarray(xSurf, dtype=np.float64)
        self._chk(self.lib.adflow_gpu_update_wall_distances(level, xSurf.ctypes.data, xSurf.size))

    def setupStateResidualMatrix(self, level=1, usePC=True, frozenTurb=False, useTurbOnly=False, viscPC=False, delta=1e-9, useAD=False,
                                 approxSA=False):
        """adjointUtils::setupStateResidualMatrix (adjointUtils.F90:7-715) without the PETSc calls: the stencil blocks stay on the
        device; jacobianBlocks() brings one block's over.  useAD = False: coloured finite differences with step delta; True: one
        forward-mode (dual-number) evaluation per colour and state variable, the exact derivative (adjointUtils.F90:227-409).
        approxSA: the SA residual of the coloured evaluations without term1 of its source (FormJacobianANK / FormJacobianANKTurb)."""
        flags = (capi.JAC_PC if usePC else 0) | (capi.JAC_FROZEN_TURB if frozenTurb else 0) \
            | (capi.JAC_TURB_ONLY if useTurbOnly else 0) | (capi.JAC_VISC_PC if viscPC else 0) | (capi.JAC_USE_AD if useAD else 0) \
            | (capi.JAC_APPROX_SA if approxSA else 0)
        self._chk(self.lib.adflow_gpu_fd_jacobian(level, flags, float(delta)))

    def releaseWorkspace(self) -> int:
        """gives the dual-number slab a forward-mode assembly keeps between calls, and the scratch arrays of jacobianMult, back to the
        device; returns the bytes released"""
        n = ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_release_workspace(ctypes.byref(n)))
        return int(n.value)

    def selftestMath(self, which: int, x, a=None):
        """the kernels' fast division / root / power forms on the arguments x (and exponents / numerators a): returns
        (plain value, dual value, dual derivative) -- csrc/internal.h, csrc/kernels_ad.hip"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        a = np.ones_like(x) if a is None else np.ascontiguousarray(np.broadcast_to(a, x.shape), dtype=np.float64)
        y = np.zeros_like(x)
        dy = np.zeros((x.size, 2))
        self._chk(self.lib.adflow_gpu_selftest_math(int(which), x.ctypes.data, a.ctypes.data, x.size, y.ctypes.data, dy.ctypes.data))
        return y, dy[:, 0].reshape(x.shape), dy[:, 1].reshape(x.shape)

    def jacobianInfo(self):
        ns, nst = ctypes.c_int32(), ctypes.c_int32()
        self._chk(self.lib.adflow_gpu_jacobian_info(ctypes.byref(ns), ctypes.byref(nst), None))
        st = np.zeros((nst.value, 3), dtype=np.int32, order="F")
        self._chk(self.lib.adflow_gpu_jacobian_info(None, None, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return ns.value, st

    def jacobianBlocks(self, nn=1, level=1, sps=1):
        """(nx, ny, nz, nState, nState, nStencil): blk(ll, l) of stencil entry s at every owned row cell"""
        ns, st = self.jacobianInfo()
        blk = self.blocks[(nn, level, sps)]
        out = np.zeros((blk.nx, blk.ny, blk.nz, ns, ns, st.shape[0]), order="F")
        self._chk(self.lib.adflow_gpu_download_jacobian(nn, level, sps, out.ctypes.data))
        return out

    def jacobianRows(self, nn=1, level=1, sps=1):
        """(nState, nState, nStencil, nx, ny, nz): the same blocks, contiguous per row cell (one MatSetValuesBlocked per cell and
        stencil entry reads nState^2 consecutive doubles)"""
        ns, st = self.jacobianInfo()
        blk = self.blocks[(nn, level, sps)]
        out = np.zeros((ns, ns, st.shape[0], blk.nx, blk.ny, blk.nz), order="F")
        self._chk(self.lib.adflow_gpu_download_jacobian_rows(nn, level, sps, out.ctypes.data))
        return out

    def jacobianMult(self, x, level=1, transpose=False):
        """y = J x, or J^T x with transpose, for the matrix setupStateResidualMatrix left on the device (MatMult on dRdw / dRdwT,
        adjointAPI.F90:741): x and y in the PETSc layout with nState variables per owned cell of the level"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        self._chk(self.lib.adflow_gpu_jacobian_mult(level, int(bool(transpose)), x.ctypes.data, y.ctypes.data, x.size))
        return y

    def jacobianMultDev(self, d_x: int, d_y: int, n: int, level=1, transpose=False):
        """the same on device pointers (the addresses of two device vectors of n doubles, e.g. torch.Tensor.data_ptr())"""
        self._chk(self.lib.adflow_gpu_jacobian_mult_dev(level, int(bool(transpose)), ctypes.c_void_p(d_x), ctypes.c_void_p(d_y), int(n)))

    def pcSetup(self, level=1):
        """block ILU(0) of the 7-point preconditioner matrix of the last setupStateResidualMatrix, one subdomain per block (the PC
        of setupStandardKSP, adjointUtils.F90:1374-1562, as PCBJACOBI / ILU(0) / natural ordering); kept until pcRelease"""
        self._chk(self.lib.adflow_gpu_pc_setup(level))

    def pcInfo(self):
        """(nState, number of hyperplanes -- level sets at fill > 0 --, bytes held) of the factor"""
        ns, npl, nb = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_pc_info(ctypes.byref(ns), ctypes.byref(npl), ctypes.byref(nb)))
        return int(ns.value), int(npl.value), int(nb.value)

    def pcSetFill(self, fill: int):
        """levels of fill (0, 1 or 2; PCFactorSetLevels) of the next pcSetup / ankPcSetup of the selected slot; a factor that exists
        keeps its own"""
        self._chk(self.lib.adflow_gpu_pc_set_fill(int(fill)))

    def pcInfo2(self):
        """(fill, entries per row: 7, 13 or 23, number of level sets) of the factor"""
        f, ne, nl = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._chk(self.lib.adflow_gpu_pc_info2(ctypes.byref(f), ctypes.byref(ne), ctypes.byref(nl)))
        return int(f.value), int(ne.value), int(nl.value)

    def pcSetCoupled(self, coupled: int):
        """0: one ILU subdomain per block (PCBJACOBI); 1: one subdomain for the level, the couplings across the block interfaces of
        this process inside M (the ASM subdomain of setupStandardKSP; fill 0, no hierarchy) -- for the next pcSetup / ankPcSetup of the
        selected slot; a factor that exists keeps its own"""
        self._chk(self.lib.adflow_gpu_pc_set_coupled(int(coupled)))

    def pcCoupledInfo(self):
        """(coupled, number of level sets, entries of M whose column lies behind a block interface) of the factor"""
        c, nl, nx = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_pc_coupled_info(ctypes.byref(c), ctypes.byref(nl), ctypes.byref(nx)))
        return int(c.value), int(nl.value), int(nx.value)

    def pcSetLevelFill(self, fill: int):
        """-1: off; 0 .. 3: the next pcSetup / ankPcSetup of the selected slot builds the ILU(fill) of the 7-point matrix of the WHOLE level
        on its general block pattern (one ASM subdomain with PCFactorSetLevels(fill), what setupStandardKSP gives one process); excludes
        pcSetCoupled(1), pcSetFill > 0 and pcSetMg > 1 in the same slot; a factor that exists keeps its own"""
        self._chk(self.lib.adflow_gpu_pc_set_level_fill(int(fill)))

    def pcLevelInfo(self):
        """(fill, longest row, blocks of the pattern over all rows, level sets, entries of the assembled matrix behind a block face,
        reused: 1 when the last setup kept the tables) of the factor over the level in the selected slot"""
        f, mr, nl, rs = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        ne, nx = ctypes.c_int64(0), ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_pc_level_info(ctypes.byref(f), ctypes.byref(mr), ctypes.byref(ne), ctypes.byref(nl), ctypes.byref(nx),
                                                    ctypes.byref(rs)))
        return int(f.value), int(mr.value), int(ne.value), int(nl.value), int(nx.value), int(rs.value)

    def pcSetOrdering(self, kind: int, perm=None):
        """the ordering of the ILU over the level (pcSetLevelFill >= 0) for the next pcSetup / ankPcSetup of the selected slot: 0 natural
        (the default), 1 the library's reverse Cuthill-McKee, 2 the caller's permutation.  perm (perm[new] = old, 0-based cell numbers
        of the PETSc layout) is handed over first when given and copied; a factor that exists keeps its own"""
        if perm is not None:
            p = np.ascontiguousarray(perm, dtype=np.int32)
            self._chk(self.lib.adflow_gpu_pc_set_ordering_perm(p.ctypes.data, p.size))
        self._chk(self.lib.adflow_gpu_pc_set_ordering(int(kind)))

    def pcDropOrderingPerm(self):
        """forget the permutation stored for the selected slot"""
        self._chk(self.lib.adflow_gpu_pc_set_ordering_perm(None, 0))

    def pcOrderingInfo(self):
        """(ordering kind, bandwidth of the assembled entries in that ordering, level sets, blocks of the pattern) of the factor of the
        selected slot; kind 0 and bandwidth -1 for a factor that is no ILU over the level"""
        k, nl = ctypes.c_int32(0), ctypes.c_int32(0)
        bw, ne = ctypes.c_int64(0), ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_pc_ordering_info(ctypes.byref(k), ctypes.byref(bw), ctypes.byref(nl), ctypes.byref(ne)))
        return int(k.value), int(bw.value), int(nl.value), int(ne.value)

    def pcOrdering(self):
        """perm[new] = old the factor of the selected slot was built with (the identity for the natural ordering)"""
        perm = np.zeros(self.pcMgInfo()[3][0], dtype=np.int32)
        self._chk(self.lib.adflow_gpu_pc_download_ordering(perm.ctypes.data, perm.size))
        return perm

    def pcSetMg(self, levels: int, nSmooth: int = 1, fillCoarse: int = 0):
        """the multigrid preconditioner of amg.F90 (precondType = 'mg') for the next pcSetup / ankPcSetup of the selected slot: `levels`
        levels of 2 x 2 x 2 aggregates per block (1: the plain factor), nSmooth Richardson iterations of the ILU smoother per level,
        fillCoarse levels of fill on the levels below the first (the first keeps pcSetFill's)"""
        self._chk(self.lib.adflow_gpu_pc_set_mg(int(levels), int(nSmooth), int(fillCoarse)))

    def pcMgInfo(self):
        """(levels, nSmooth, fillCoarse, cells of every level) of the factor or hierarchy of the selected slot"""
        lv, nsm, fc = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._chk(self.lib.adflow_gpu_pc_mg_info(ctypes.byref(lv), ctypes.byref(nsm), ctypes.byref(fc), None))
        cells = np.zeros(lv.value, dtype=np.int64)
        self._chk(self.lib.adflow_gpu_pc_mg_info(None, None, None, cells.ctypes.data))
        return int(lv.value), int(nsm.value), int(fc.value), tuple(int(c) for c in cells)

    def pcSetIts(self, outer: int = 1, inner: int = 1, innerCoarse: int = 1):
        """the Richardson iterations of setupStandardKSP around the factor for the next pcSetup / ankPcSetup of the selected slot: `outer`
        (outerPreconIts: on the 7-point matrix of the whole level, columns behind block faces included), `inner` (innerPreconIts: on
        the matrix the factor was built from; level 1 of a hierarchy), innerCoarse (innerPreconItsCoarse: the levels below); a
        factor that exists keeps its own"""
        self._chk(self.lib.adflow_gpu_pc_set_its(int(outer), int(inner), int(innerCoarse)))

    def pcItsInfo(self):
        """(outer, inner, innerCoarse, bytes of the owned copy of the matrix of the level and its tables: 0 when none is held) of
        the factor of the selected slot"""
        o, i, c, nb = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_pc_its_info(ctypes.byref(o), ctypes.byref(i), ctypes.byref(c), ctypes.byref(nb)))
        return int(o.value), int(i.value), int(c.value), int(nb.value)

    def pcMgMatrix(self, mgLevel: int, nn=1, level=1, sps=1):
        """(nx_l, ny_l, nz_l, nState, nState, 7): the blocks of block nn on level mgLevel of the hierarchy, laid out as jacobianBlocks;
        mgLevel = 1 is the owned copy of the in-block blocks (T included)"""
        ns = self.pcInfo()[0]
        blk = self.blocks[(nn, level, sps)]
        d = [blk.nx, blk.ny, blk.nz]
        for _ in range(int(mgLevel) - 1):
            d = [(n + 1) // 2 for n in d]
        out = np.zeros((d[0], d[1], d[2], ns, ns, 7), order="F")
        self._chk(self.lib.adflow_gpu_pc_mg_download(int(mgLevel), nn, out.ctypes.data))
        return out

    def pcApply(self, r, level=1, transpose=False):
        """z = M^-1 r, or M^-T r with transpose, for the factor of pcSetup; vectors as for jacobianMult"""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        self._chk(self.lib.adflow_gpu_pc_apply(level, int(bool(transpose)), r.ctypes.data, z.ctypes.data, r.size))
        return z

    def pcApplyDev(self, d_r: int, d_z: int, n: int, level=1, transpose=False):
        """the same on device pointers (e.g. torch.Tensor.data_ptr())"""
        self._chk(self.lib.adflow_gpu_pc_apply_dev(level, int(bool(transpose)), ctypes.c_void_p(d_r), ctypes.c_void_p(d_z), int(n)))

    def pcRelease(self) -> int:
        """frees the factor; returns the bytes released (0 when there was none)"""
        n = ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_pc_release(ctypes.byref(n)))
        return int(n.value)

    def gmresSolve(self, b, level=1, transpose=False, restart=50, maxIts=200, rtol=1e-8, atol=0.0, x0=None):
        """right-preconditioned GMRES(restart) on the matrix assembled last with the factor of pcSetup (KSPSolve of solveAdjoint,
        adjointAPI.F90:661-863); returns (x, iterations, initial residual norm, true residual norm of x)"""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64, order="C", copy=True)
        its, r0, rn = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(self.lib.adflow_gpu_gmres_solve(level, int(bool(transpose)), b.ctypes.data, x.ctypes.data, b.size, int(restart),
                                                  int(maxIts), float(rtol), float(atol), int(x0 is not None), ctypes.byref(its),
                                                  ctypes.byref(r0), ctypes.byref(rn)))
        return x, int(its.value), float(r0.value), float(rn.value)

    def gmresSolveDev(self, d_b: int, d_x: int, n: int, level=1, transpose=False, restart=50, maxIts=200, rtol=1e-8, atol=0.0,
                      useGuess=False):
        """the same on device pointers; returns (iterations, initial residual norm, true residual norm)"""
        its, r0, rn = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(self.lib.adflow_gpu_gmres_solve_dev(level, int(bool(transpose)), ctypes.c_void_p(d_b), ctypes.c_void_p(d_x), int(n),
                                                      int(restart), int(maxIts), float(rtol), float(atol), int(bool(useGuess)),
                                                      ctypes.byref(its), ctypes.byref(r0), ctypes.byref(rn)))
        return int(its.value), float(r0.value), float(rn.value)

    # ---- matrix-free exact products by forward mode (dRdwMatMult, adjointAPI.F90:1050-1128): no assembled matrix
    @staticmethod
    def _jacFreeFlags(usePC, frozenTurb, useTurbOnly, viscPC, approxSA):
        return (capi.JAC_PC if usePC else 0) | (capi.JAC_FROZEN_TURB if frozenTurb else 0) | (capi.JAC_TURB_ONLY if useTurbOnly else 0) \
            | (capi.JAC_VISC_PC if viscPC else 0) | (capi.JAC_APPROX_SA if approxSA else 0)

    def jacFreeMult(self, x, level=1, usePC=False, frozenTurb=False, useTurbOnly=False, viscPC=False, approxSA=False):
        """y = (dR/dw) x by ONE forward-mode evaluation seeded with x, about the state on the device: what jacobianMult returns after
        setupStateResidualMatrix(level, usePC, ..., useAD=True), without the matrix.  Vectors as for jacobianMult"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        flags = self._jacFreeFlags(usePC, frozenTurb, useTurbOnly, viscPC, approxSA)
        self._chk(self.lib.adflow_gpu_jacfree_mult(level, flags, x.ctypes.data, y.ctypes.data, x.size))
        return y

    def jacFreeMultDev(self, d_x: int, d_y: int, n: int, level=1, usePC=False, frozenTurb=False, useTurbOnly=False, viscPC=False,
                       approxSA=False):
        """the same on device pointers (e.g. torch.Tensor.data_ptr())"""
        flags = self._jacFreeFlags(usePC, frozenTurb, useTurbOnly, viscPC, approxSA)
        self._chk(self.lib.adflow_gpu_jacfree_mult_dev(level, flags, ctypes.c_void_p(d_x), ctypes.c_void_p(d_y), int(n)))

    def jacFreeSolve(self, b, level=1, restart=50, maxIts=200, rtol=1e-8, atol=0.0, x0=None, usePC=False, frozenTurb=False,
                     useTurbOnly=False, viscPC=False, approxSA=False):
        """right-preconditioned GMRES(restart) on the matrix-free product with the factor of pcSetup, never transposed (the KSP of
        solveDirectForRHS on the shell dRdwT); returns (x, iterations, initial residual norm, true residual norm of x)"""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64, order="C", copy=True)
        its, r0, rn = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        flags = self._jacFreeFlags(usePC, frozenTurb, useTurbOnly, viscPC, approxSA)
        self._chk(self.lib.adflow_gpu_jacfree_solve(level, flags, b.ctypes.data, x.ctypes.data, b.size, int(restart), int(maxIts),
                                                    float(rtol), float(atol), int(x0 is not None), ctypes.byref(its), ctypes.byref(r0),
                                                    ctypes.byref(rn)))
        return x, int(its.value), float(r0.value), float(rn.value)

    def jacFreeSolveDev(self, d_b: int, d_x: int, n: int, level=1, restart=50, maxIts=200, rtol=1e-8, atol=0.0, useGuess=False,
                        usePC=False, frozenTurb=False, useTurbOnly=False, viscPC=False, approxSA=False):
        """the same on device pointers; returns (iterations, initial residual norm, true residual norm)"""
        its, r0, rn = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        flags = self._jacFreeFlags(usePC, frozenTurb, useTurbOnly, viscPC, approxSA)
        self._chk(self.lib.adflow_gpu_jacfree_solve_dev(level, flags, ctypes.c_void_p(d_b), ctypes.c_void_p(d_x), int(n), int(restart),
                                                        int(maxIts), float(rtol), float(atol), int(bool(useGuess)), ctypes.byref(its),
                                                        ctypes.byref(r0), ctypes.byref(rn)))
        return int(its.value), float(r0.value), float(rn.value)

    # ---- several right-hand sides at once: columns as the rows of a C-contiguous (nvec, n) array, so ld = n
    @staticmethod
    def _columns(A):
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2:
            raise ValueError("the columns of a multi entry are the rows of an array of shape (nvec, n)")
        return A

    def jacobianMultMulti(self, X, level=1, transpose=False):
        """Y[c] = J X[c] (J^T X[c]) for the nvec rows of X in one pass over the matrix per group of 4 (jacobianMult per column)"""
        X = self._columns(X)
        Y = np.zeros_like(X)
        nvec, n = X.shape
        self._chk(self.lib.adflow_gpu_jacobian_mult_multi(level, int(bool(transpose)), nvec, X.ctypes.data, n, Y.ctypes.data, n, n))
        return Y

    def jacobianMultMultiDev(self, d_X: int, ldx: int, d_Y: int, ldy: int, nvec: int, n: int, level=1, transpose=False):
        """the same on device pointers: column c at d_X + 8 c ldx bytes (ld >= n)"""
        self._chk(self.lib.adflow_gpu_jacobian_mult_multi_dev(level, int(bool(transpose)), int(nvec), ctypes.c_void_p(d_X), int(ldx),
                                                              ctypes.c_void_p(d_Y), int(ldy), int(n)))

    def pcApplyMulti(self, R, level=1, transpose=False):
        """Z[c] = M^-1 R[c] (M^-T R[c]) for the nvec rows of R through the level sets once per group of 4 (pcApply per column)"""
        R = self._columns(R)
        Z = np.zeros_like(R)
        nvec, n = R.shape
        self._chk(self.lib.adflow_gpu_pc_apply_multi(level, int(bool(transpose)), nvec, R.ctypes.data, n, Z.ctypes.data, n, n))
        return Z

    def pcApplyMultiDev(self, d_R: int, ldr: int, d_Z: int, ldz: int, nvec: int, n: int, level=1, transpose=False):
        """the same on device pointers"""
        self._chk(self.lib.adflow_gpu_pc_apply_multi_dev(level, int(bool(transpose)), int(nvec), ctypes.c_void_p(d_R), int(ldr),
                                                         ctypes.c_void_p(d_Z), int(ldz), int(n)))

    def gmresSolveMulti(self, B, level=1, transpose=False, restart=50, maxIts=200, rtol=1e-8, atol=0.0, x0=None):
        """gmresSolve for the nvec rows of B in lock-step; returns (X, its[], rnorm0[], rnorm[]), every column as its own gmresSolve
        would leave it (x0: an array like B with the initial guess of every column)"""
        B = self._columns(B)
        X = np.zeros_like(B) if x0 is None else np.array(x0, dtype=np.float64, order="C", copy=True)
        assert X.shape == B.shape
        nvec, n = B.shape
        its, r0, rn = np.zeros(nvec, dtype=np.int32), np.zeros(nvec), np.zeros(nvec)
        self._chk(self.lib.adflow_gpu_gmres_solve_multi(level, int(bool(transpose)), nvec, B.ctypes.data, n, X.ctypes.data, n, n,
                                                        int(restart), int(maxIts), float(rtol), float(atol), int(x0 is not None),
                                                        its.ctypes.data, r0.ctypes.data, rn.ctypes.data))
        return X, its, r0, rn

    def gmresSolveMultiDev(self, d_B: int, ldb: int, d_X: int, ldx: int, nvec: int, n: int, level=1, transpose=False, restart=50,
                           maxIts=200, rtol=1e-8, atol=0.0, useGuess=False):
        """the same on device pointers; returns (its[], rnorm0[], rnorm[])"""
        its, r0, rn = np.zeros(nvec, dtype=np.int32), np.zeros(nvec), np.zeros(nvec)
        self._chk(self.lib.adflow_gpu_gmres_solve_multi_dev(level, int(bool(transpose)), int(nvec), ctypes.c_void_p(d_B), int(ldb),
                                                            ctypes.c_void_p(d_X), int(ldx), int(n), int(restart), int(maxIts),
                                                            float(rtol), float(atol), int(bool(useGuess)), its.ctypes.data,
                                                            r0.ctypes.data, rn.ctypes.data))
        return its, r0, rn

    def pcSelect(self, slot: int):
        """the factor slot (0 or 1) pcSetup, ankPcSetup, pcApply, pcInfo, pcRelease, gmresSolve and ankSolve act on"""
        self._chk(self.lib.adflow_gpu_pc_select(int(slot)))

    # ---- ANKStep / ANKTurbSolveKSP (NKSolvers.F90:3337-4112); vectors carry nState = nw (coupled), 1 (turb) or 5 variables per cell
    @staticmethod
    def _ankFlags(coupled=False, dissApprox=False, viscApprox=False, useBlockettes=False, turb=False, approxSA=False, turbFirstOrder=False):
        return (capi.ANK_COUPLED if coupled else 0) | (capi.RES_DISS_APPROX if dissApprox else 0) \
            | (capi.RES_VISC_APPROX if viscApprox else 0) | (capi.RES_UPWIND_FIRST_ORDER if useBlockettes else 0) \
            | (capi.ANK_TURB if turb else 0) | (capi.RES_APPROX_SA if approxSA else 0) \
            | (capi.RES_TURB_FIRST_ORDER if turbFirstOrder else 0)

    def ankNState(self, coupled=False, turb=False):
        if turb:
            return 1
        return next(b.nw for (nn, lv, sps), b in self.blocks.items() if lv == 1) if coupled else 5

    def _ankCells(self):
        return sum(b.nx * b.ny * b.nz for (nn, lv, sps), b in self.blocks.items() if lv == 1)

    def ankSetW(self, w, coupled=False, turb=False):
        """setWANK(wVec, 1, nState) / setWANK(wVecTurb, nt1, nt2): the owned cells, no clipping"""
        w = np.ascontiguousarray(w, dtype=np.float64)
        self._chk(self.lib.adflow_gpu_ank_set_w(w.ctypes.data, w.size, self._ankFlags(coupled, turb=turb)))

    def ankGetR(self, coupled=False, turb=False):
        """setRVecANK (decoupled) / setRVec (coupled) / setRVecANKTurb (turb) of the residual on the device"""
        n = self.ankNState(coupled, turb) * self._ankCells()
        r = np.zeros(n)
        self._chk(self.lib.adflow_gpu_ank_get_r(r.ctypes.data, n, self._ankFlags(coupled, turb=turb)))
        return r

    def ankSetWDev(self, d_w: int, n: int, flags=0):
        """ankSetW on a device pointer; flags: ADFLOW_ANK_COUPLED / ADFLOW_ANK_TURB (_ankFlags)"""
        self._chk(self.lib.adflow_gpu_ank_set_w_dev(ctypes.c_void_p(d_w), int(n), int(flags)))

    def ankGetRDev(self, d_r: int, n: int, flags=0):
        """ankGetR into a device pointer"""
        self._chk(self.lib.adflow_gpu_ank_get_r_dev(ctypes.c_void_p(d_r), int(n), int(flags)))

    def ankTimeStep(self, cfl, turbCFLScale=1.0, coupled=False, level=1, turb=False):
        """computeTimeStepMat for ANK_charTimeStepType = 'None' from the dtl on the device; turb: the diagonal of the turbulence KSP"""
        self._chk(self.lib.adflow_gpu_ank_time_step(level, float(cfl), float(turbCFLScale), self._ankFlags(coupled, turb=turb)))

    def ankTimeStepBlocks(self, nn=1, coupled=False, level=1, turb=False):
        """the dense blocks of T of block nn, (nState, nState, nx, ny, nz)"""
        blk = self.blocks[(nn, level, 1)]
        ns = self.ankNState(coupled, turb)
        out = np.zeros((ns, ns, blk.nx, blk.ny, blk.nz), order="F")
        if turb:
            self._chk(self.lib.adflow_gpu_ank_download_time_step_turb(nn, out.ctypes.data, capi.ANK_TURB))
        else:
            self._chk(self.lib.adflow_gpu_ank_download_time_step(nn, out.ctypes.data))
        return out

    def ankPcSetup(self, level=1):
        """ILU(0) of dRdwPre + timeStepMat into the selected factor slot (FormJacobianANK; FormJacobianANKTurb for a useTurbOnly matrix)"""
        self._chk(self.lib.adflow_gpu_ank_pc_setup(level))

    def ankSetBase(self, w, coupled=False, dissApprox=False, viscApprox=False, useBlockettes=False, turb=False, approxSA=False,
                   turbFirstOrder=False):
        """formFunction_mf[_turb](wVec, baseRes) + MatMFFDSetBase: the state from w, r0 = R(w) kept on the device"""
        w = np.ascontiguousarray(w, dtype=np.float64)
        self._chk(self.lib.adflow_gpu_ank_set_base(w.ctypes.data, w.size, self._ankFlags(coupled, dissApprox, viscApprox, useBlockettes, turb,
                                                                                          approxSA, turbFirstOrder)))

    def ankSetBaseDev(self, d_w: int, n: int, flags=0):
        """ankSetBase on a device pointer; flags: the kind and the residual flags (_ankFlags)"""
        self._chk(self.lib.adflow_gpu_ank_set_base_dev(ctypes.c_void_p(d_w), int(n), int(flags)))

    def ankMult(self, v):
        """y = (R(w + h v) - r0) / h + T v with the MATMFFD_DS step h, on the base set last; the device state is the perturbed one
        afterwards"""
        v = np.ascontiguousarray(v, dtype=np.float64)
        y = np.zeros_like(v)
        self._chk(self.lib.adflow_gpu_ank_mult(v.ctypes.data, y.ctypes.data, v.size))
        return y

    def ankSelectBase(self, turb=False):
        """the kind (flow / turbulence) whose base ankMult, ankSolve and ankLastH act on; by default the one set last"""
        self._chk(self.lib.adflow_gpu_ank_select_base(capi.ANK_TURB if turb else 0))

    def ankMultDev(self, d_v: int, d_y: int, n: int):
        self._chk(self.lib.adflow_gpu_ank_mult_dev(ctypes.c_void_p(d_v), ctypes.c_void_p(d_y), int(n)))

    def ankLastH(self) -> float:
        h = ctypes.c_double(0.0)
        self._chk(self.lib.adflow_gpu_ank_last_h(ctypes.byref(h)))
        return float(h.value)

    def ankSolve(self, b, level=1, restart=50, maxIts=200, rtol=1e-8, atol=0.0):
        """KSPSolve(ANK_KSP, rVec, deltaW): GMRES on ankMult with the selected factor slot as right preconditioner, from zero; returns
        (x, iterations, initial residual norm, true residual norm of x)"""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        its, r0, rn = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(self.lib.adflow_gpu_ank_solve(level, b.ctypes.data, x.ctypes.data, b.size, int(restart), int(maxIts), float(rtol),
                                                float(atol), ctypes.byref(its), ctypes.byref(r0), ctypes.byref(rn)))
        return x, int(its.value), float(r0.value), float(rn.value)

    def ankSolveDev(self, d_b: int, d_x: int, n: int, level=1, restart=50, maxIts=200, rtol=1e-8, atol=0.0):
        its, r0, rn = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(self.lib.adflow_gpu_ank_solve_dev(level, ctypes.c_void_p(d_b), ctypes.c_void_p(d_x), int(n), int(restart), int(maxIts),
                                                    float(rtol), float(atol), ctypes.byref(its), ctypes.byref(r0), ctypes.byref(rn)))
        return int(its.value), float(r0.value), float(rn.value)

    def ankPhysicalityCheck(self, w, dw, lambda0=1.0, coupled=False, physLSTol=0.2, physLSTolTurb=0.99, stepFactor=1.0, stepMin=0.01,
                            turb=False):
        """physicalityCheckANK / physicalityCheckANKTurb: returns (lambda, dw with the clipped turbulence entries)"""
        w = np.ascontiguousarray(w, dtype=np.float64)
        dw = np.array(dw, dtype=np.float64, order="C", copy=True)
        lam = ctypes.c_double(float(lambda0))
        self._chk(self.lib.adflow_gpu_ank_physicality_check(w.ctypes.data, dw.ctypes.data, w.size, self._ankFlags(coupled, turb=turb),
                                                            float(physLSTol), float(physLSTolTurb), float(stepFactor), float(stepMin),
                                                            ctypes.byref(lam)))
        return float(lam.value), dw

    def ankPhysicalityCheckDev(self, d_w: int, d_dw: int, n: int, flags=0, lambda0=1.0, physLSTol=0.2, physLSTolTurb=0.99, stepFactor=1.0,
                               stepMin=0.01) -> float:
        """the same on device pointers: d_dw is clipped in place, lambda comes back (synchronous: it goes to the host)"""
        lam = ctypes.c_double(float(lambda0))
        self._chk(self.lib.adflow_gpu_ank_physicality_check_dev(ctypes.c_void_p(d_w), ctypes.c_void_p(d_dw), int(n), int(flags), float(physLSTol),
                                                                float(physLSTolTurb), float(stepFactor), float(stepMin), ctypes.byref(lam)))
        return float(lam.value)

    def ankUnsteadyRes(self, dW, omega, coupled=False, turb=False, dissApprox=False, viscApprox=False, useBlockettes=False, approxSA=False,
                       turbFirstOrder=False):
        """computeUnsteadyResANK / ...Turb on the state ankSetW left: returns (R(w) - omega T dW, its 2-norm)"""
        dW = np.ascontiguousarray(dW, dtype=np.float64)
        r = np.zeros_like(dW)
        nrm = ctypes.c_double(0.0)
        flags = self._ankFlags(coupled, dissApprox, viscApprox, useBlockettes, turb, approxSA, turbFirstOrder)
        self._chk(self.lib.adflow_gpu_ank_unsteady_res(dW.ctypes.data, float(omega), r.ctypes.data, dW.size, flags, ctypes.byref(nrm)))
        return r, float(nrm.value)

    def ankUnsteadyResDev(self, d_dW: int, omega, d_r: int, n: int, flags=0, norm=True):
        """the same on device pointers; norm=False skips the reduction (and the synchronisation) and returns None"""
        nrm = ctypes.c_double(0.0)
        self._chk(self.lib.adflow_gpu_ank_unsteady_res_dev(ctypes.c_void_p(d_dW), float(omega), ctypes.c_void_p(d_r), int(n), int(flags),
                                                           ctypes.byref(nrm) if norm else None))
        return float(nrm.value) if norm else None

    def ankRelease(self) -> int:
        """frees both T, the base vectors and the sums; returns the bytes released"""
        n = ctypes.c_int64(0)
        self._chk(self.lib.adflow_gpu_ank_release(ctypes.byref(n)))
        return int(n.value)

    def blocketteRes(self, level=1, updateIntermed=True, flowRes=True, turbRes=True, dissApprox=False, viscApprox=False,
                     useBlockettes=False, halo=False, closures=False, approxSA=False, turbFirstOrder=False):
        """halo: also the part of blocketteRes in front of the core -- boundary conditions and whalo2 (ADFLOW_RES_HALO);
        closures: and the derived values in front of those -- computePressureSimple, computeLamViscosity, computeEddyViscosity
        (ADFLOW_RES_CLOSURES, blockette.F90:199-203).  Both = the reference's whole blocketteRes.  approxSA: term1 of the SA source
        is zero (sa.F90:296); turbFirstOrder: orderTurb = firstOrder for this call only."""
        flags = (capi.RES_UPDATE_INTERMED if updateIntermed else 0) | (capi.RES_FLOW if flowRes else 0) \
            | (capi.RES_TURB if turbRes else 0) | (32 if dissApprox else 0) | (64 if viscApprox else 0) \
            | (128 if useBlockettes else 0) | (capi.RES_HALO if halo else 0) | (capi.RES_CLOSURES if closures else 0) \
            | (capi.RES_APPROX_SA if approxSA else 0) | (capi.RES_TURB_FIRST_ORDER if turbFirstOrder else 0)
        self._chk(self.lib.adflow_gpu_block_res(level, flags))

    def bc_register(self, faces, nViscBocos: int = 0, nn: int = 1, level: int = 1, sps: int = 1):
        """flowDoms(nn,level,sps)%BCType/BCFaceID/BCData -> device.  `faces`: list of dicts with bcType, faceID,
        icBeg, icEnd, jcBeg, jcEnd and the BCData members (Fortran-order float64 arrays) the kind needs."""
        arr = (capi.AdflowBcSubface * max(len(faces), 1))()
        for m, f in enumerate(faces):
            for k in ("bcType", "faceID", "icBeg", "icEnd", "jcBeg", "jcEnd"):
                setattr(arr[m], k, int(f[k]))
            arr[m].subsonicInletTreatment = int(f.get("subsonicInletTreatment", 0))
            if f.get("symNorm") is not None:
                for q in range(3):
                    arr[m].symNorm[q] = float(f["symNorm"][q])
            for k in capi.BC_ARRAYS:
                a = f.get(k)
                if a is not None:
                    assert a.flags["F_CONTIGUOUS"] and a.dtype == np.float64, k
                    setattr(arr[m], k, a.ctypes.data)
        self._chk(self.lib.adflow_gpu_bc_register(nn, level, sps, len(faces), int(nViscBocos), arr))

    def wall_stress(self, shape, mm: int, nn: int = 1, level: int = 1, sps: int = 1):
        """viscSubface(mm)%tau, %q of viscous subface mm (1-based) over its owned face cells `shape` = (n1, n2)"""
        tau = np.zeros(tuple(shape) + (6,), order="F")
        q = np.zeros(tuple(shape) + (3,), order="F")
        self._chk(self.lib.adflow_gpu_download_wall_stress(nn, level, sps, mm, tau.ctypes.data, q.ctypes.data))
        return tau, q

    # ---- surface integration (surfaceIntegrations.F90: wallIntegrationFace, computeCpMinFamily) ----
    @staticmethod
    def wallPar(MachCoef, pointRef=(0.0, 0.0, 0.0), momentAxis=((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)), velDirFreeStream=(1.0, 0.0, 0.0),
                sepSensorOffset=0.0, sepSensorSharpness=10.0, computeCavitation=False, cavitationnumber=1.4, cavSensorOffset=0.0,
                cavSensorSharpness=10.0, cavExponent=0, cpmin_rho=100.0, cpmin_family=0.0):
        """the parameter array of wallIntegrate; momentAxis = (first point, second point); the defaults of the sensors are those of
        inputCostFunctions / inputPhysics"""
        par = np.zeros(capi.WALLINT_NPAR)
        par[capi.WALLINT_MACHCOEF] = MachCoef
        par[capi.WALLINT_POINTREF:capi.WALLINT_POINTREF + 3] = pointRef
        par[capi.WALLINT_MOMENTAXIS:capi.WALLINT_MOMENTAXIS + 6] = np.asarray(momentAxis, dtype=np.float64).reshape(6)
        par[capi.WALLINT_VELDIRFREESTREAM:capi.WALLINT_VELDIRFREESTREAM + 3] = velDirFreeStream
        par[capi.WALLINT_SEPSENSOROFFSET], par[capi.WALLINT_SEPSENSORSHARPNESS] = sepSensorOffset, sepSensorSharpness
        par[capi.WALLINT_COMPUTECAVITATION], par[capi.WALLINT_CAVITATIONNUMBER] = float(bool(computeCavitation)), cavitationnumber
        par[capi.WALLINT_CAVSENSOROFFSET], par[capi.WALLINT_CAVSENSORSHARPNESS] = cavSensorOffset, cavSensorSharpness
        par[capi.WALLINT_CAVEXPONENT], par[capi.WALLINT_CPMIN_RHO], par[capi.WALLINT_CPMIN_FAMILY] = cavExponent, cpmin_rho, cpmin_family
        return par

    @staticmethod
    def _famLists(groups):
        """groups: None (one group of every wall subface) or a list of family lists -> (nGroups, famLists (nGroups, ldFam) F-order, ldFam)"""
        if groups is None:
            return 0, None, 0
        ld = 1 + max([len(g) for g in groups] + [0])
        fl = np.zeros((max(len(groups), 1), ld), np.int32, order="F")
        for g, fams in enumerate(groups):
            fl[g, 0] = len(fams)
            fl[g, 1:1 + len(fams)] = fams
        return len(groups), fl, ld

    def bcSetFamilies(self, famID, iblank=None, nn: int = 1, level: int = 1, sps: int = 1):
        """BCData(mm)%famID of the registered subfaces of a block and, optionally, their face blanking: iblank = None or a list with, per
        subface, None (all ones) or an int8 array over the owned face cells"""
        fam = np.ascontiguousarray(famID, np.int32)
        ptrs = None
        keep = []
        if iblank is not None:
            assert len(iblank) == fam.size
            ptrs = (ctypes.c_void_p * max(fam.size, 1))()
            for m, a in enumerate(iblank):
                if a is not None:
                    a = np.asfortranarray(a, dtype=np.int8)
                    keep.append(a)
                    ptrs[m] = a.ctypes.data
        self._chk(self.lib.adflow_gpu_bc_set_families(nn, level, sps, int(fam.size), fam.ctypes.data, ptrs))

    def wallIntegrate(self, par, groups=None, level: int = 1):
        """localValues(1:63) of every family group (entries 0..62) and the group's minimum of Cp (entry 63): an (nGroups, 64) array;
        groups = None: one group holding every wall subface"""
        par = np.ascontiguousarray(par, dtype=np.float64)
        assert par.size == capi.WALLINT_NPAR
        n, fl, ld = self._famLists(groups)
        out = np.zeros((max(n, 1) if groups is None else n, capi.WALLINT_STRIDE))
        if groups is not None and n == 0:
            return out
        self._chk(self.lib.adflow_gpu_wall_integrate(level, par.ctypes.data, n, None if fl is None else fl.ctypes.data, ld, out.ctypes.data))
        return out

    def wallIntegrateDev(self, par, d_out: int, groups=None, level: int = 1):
        """the same into a device array of nGroups x 64 doubles; honours set_async"""
        par = np.ascontiguousarray(par, dtype=np.float64)
        assert par.size == capi.WALLINT_NPAR
        n, fl, ld = self._famLists(groups)
        self._chk(self.lib.adflow_gpu_wall_integrate_dev(level, par.ctypes.data, n, None if fl is None else fl.ctypes.data, ld,
                                                         ctypes.c_void_p(d_out)))

    # ---- derivatives of the integration with respect to the state (master_d / master_b for the wall subfaces) ----
    def _wallDerivArgs(self, par, groups, frozenTurb, useTurbOnly):
        par = np.ascontiguousarray(par, dtype=np.float64)
        assert par.size == capi.WALLINT_NPAR
        n, fl, ld = self._famLists(groups)
        flags = self._jacFreeFlags(False, frozenTurb, useTurbOnly, False, False)
        return par, n, fl, None if fl is None else fl.ctypes.data, ld, flags

    def wallIntegrateFwd(self, x, par, groups=None, level: int = 1, frozenTurb=False, useTurbOnly=False, values=True):
        """(out, outDot), each (nGroups, 64): the integration and its derivative in the direction x (a vector in the layout of
        jacFreeMult) by one forward-mode pass over the front of the evaluation; values=False: out is not asked for (None)"""
        par, n, fl, pfl, ld, flags = self._wallDerivArgs(par, groups, frozenTurb, useTurbOnly)
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros((max(n, 1), capi.WALLINT_STRIDE)) if values else None
        dot = np.zeros((max(n, 1), capi.WALLINT_STRIDE))
        self._chk(self.lib.adflow_gpu_wall_integrate_fwd(level, flags, x.ctypes.data, x.size, par.ctypes.data, n, pfl, ld,
                                                         None if out is None else out.ctypes.data, dot.ctypes.data))
        return out, dot

    def wallIntegrateFwdDev(self, d_x: int, n: int, par, d_out: int, d_outDot: int, groups=None, level: int = 1, frozenTurb=False,
                            useTurbOnly=False):
        """the same on device pointers (d_out may be 0); honours set_async"""
        par, ng, fl, pfl, ld, flags = self._wallDerivArgs(par, groups, frozenTurb, useTurbOnly)
        self._chk(self.lib.adflow_gpu_wall_integrate_fwd_dev(level, flags, ctypes.c_void_p(d_x), int(n), par.ctypes.data, ng, pfl, ld,
                                                             ctypes.c_void_p(d_out) if d_out else None, ctypes.c_void_p(d_outDot)))

    def wallIntegrateBwd(self, outBar, n: int, par, groups=None, level: int = 1, frozenTurb=False, useTurbOnly=False, ld=None, fill=0.0):
        """outBar: (nRhs, nGroups, 64) weights (or (nGroups, 64) for one set) -> wbar (nRhs, ld), row r = sum outBar[r] d out / d w in its
        first n entries: the right-hand sides of the adjoint.  ld > n leaves a padding the call does not touch (it keeps `fill`)"""
        par, ng, fl, pfl, ldf, flags = self._wallDerivArgs(par, groups, frozenTurb, useTurbOnly)
        ob = np.ascontiguousarray(outBar, dtype=np.float64).reshape(-1, max(ng, 1), capi.WALLINT_STRIDE)
        ld = int(n) if ld is None else int(ld)
        wbar = np.full((ob.shape[0], max(ld, 1)), float(fill))
        self._chk(self.lib.adflow_gpu_wall_integrate_bwd(level, flags, par.ctypes.data, ng, pfl, ldf, ob.ctypes.data, ob.shape[0],
                                                         wbar.ctypes.data, int(n), ld))
        return wbar

    def wallIntegrateBwdDev(self, outBar, d_wbar: int, n: int, ld: int, par, groups=None, level: int = 1, frozenTurb=False,
                            useTurbOnly=False):
        """the same into device vectors ld doubles apart (outBar stays a host array); honours set_async"""
        par, ng, fl, pfl, ldf, flags = self._wallDerivArgs(par, groups, frozenTurb, useTurbOnly)
        ob = np.ascontiguousarray(outBar, dtype=np.float64).reshape(-1, max(ng, 1), capi.WALLINT_STRIDE)
        self._chk(self.lib.adflow_gpu_wall_integrate_bwd_dev(level, flags, par.ctypes.data, ng, pfl, ldf, ob.ctypes.data, ob.shape[0],
                                                             ctypes.c_void_p(d_wbar), int(n), int(ld)))

    def wallForces(self, shape, mm: int, nn: int = 1, level: int = 1, sps: int = 1):
        """BCData(mm)%Fp, %Fv, %area of wall subface mm (1-based) as the last wallIntegrate left them, over its owned face cells
        `shape` = (n1, n2)"""
        Fp = np.zeros(tuple(shape) + (3,), order="F")
        Fv = np.zeros(tuple(shape) + (3,), order="F")
        area = np.zeros(tuple(shape), order="F")
        self._chk(self.lib.adflow_gpu_download_wall_forces(nn, level, sps, mm, Fp.ctypes.data, Fv.ctypes.data, area.ctypes.data))
        return Fp, Fv, area

    # ---- flow integration (surfaceIntegrations.F90: flowIntegrationFace) and its derivatives with respect to the state ----
    @staticmethod
    def flowPar(rhoRef, rGasDim, pointRef=(0.0, 0.0, 0.0), internalFlow=False):
        """the parameter array of flowIntegrate: what flowIntegrationFace reads and set_options does not carry"""
        par = np.zeros(capi.FLOWINT_NPAR)
        par[capi.FLOWINT_POINTREF:capi.FLOWINT_POINTREF + 3] = pointRef
        par[capi.FLOWINT_INTERNALFLOW], par[capi.FLOWINT_RHOREF], par[capi.FLOWINT_RGASDIM] = float(bool(internalFlow)), rhoRef, rGasDim
        return par

    def _flowArgs(self, par, groups, frozenTurb=False, useTurbOnly=False):
        par = np.ascontiguousarray(par, dtype=np.float64)
        assert par.size == capi.FLOWINT_NPAR
        n, fl, ld = self._famLists(groups)
        flags = self._jacFreeFlags(False, frozenTurb, useTurbOnly, False, False)
        return par, n, fl, None if fl is None else fl.ctypes.data, ld, flags

    def flowIntegrate(self, par, groups=None, level: int = 1):
        """localValues(1:63) of flowIntegrationFace over the in- and outflow subfaces of every family group: an (nGroups, 64) array to
        be added to that of wallIntegrate; groups = None: one group holding every in- and outflow subface"""
        par, n, fl, pfl, ld, _ = self._flowArgs(par, groups)
        out = np.zeros((max(n, 1) if groups is None else n, capi.WALLINT_STRIDE))
        if groups is not None and n == 0:
            return out
        self._chk(self.lib.adflow_gpu_flow_integrate(level, par.ctypes.data, n, pfl, ld, out.ctypes.data))
        return out

    def flowIntegrateDev(self, par, d_out: int, groups=None, level: int = 1):
        """the same into a device array of nGroups x 64 doubles; honours set_async"""
        par, n, fl, pfl, ld, _ = self._flowArgs(par, groups)
        self._chk(self.lib.adflow_gpu_flow_integrate_dev(level, par.ctypes.data, n, pfl, ld, ctypes.c_void_p(d_out)))

    def flowIntegrateFwd(self, x, par, groups=None, level: int = 1, frozenTurb=False, useTurbOnly=False, values=True):
        """(out, outDot) as wallIntegrateFwd, for the in- and outflow subfaces"""
        par, n, fl, pfl, ld, flags = self._flowArgs(par, groups, frozenTurb, useTurbOnly)
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros((max(n, 1), capi.WALLINT_STRIDE)) if values else None
        dot = np.zeros((max(n, 1), capi.WALLINT_STRIDE))
        self._chk(self.lib.adflow_gpu_flow_integrate_fwd(level, flags, x.ctypes.data, x.size, par.ctypes.data, n, pfl, ld,
                                                         None if out is None else out.ctypes.data, dot.ctypes.data))
        return out, dot

    def flowIntegrateFwdDev(self, d_x: int, n: int, par, d_out: int, d_outDot: int, groups=None, level: int = 1, frozenTurb=False,
                            useTurbOnly=False):
        """the same on device pointers (d_out may be 0); honours set_async"""
        par, ng, fl, pfl, ld, flags = self._flowArgs(par, groups, frozenTurb, useTurbOnly)
        self._chk(self.lib.adflow_gpu_flow_integrate_fwd_dev(level, flags, ctypes.c_void_p(d_x), int(n), par.ctypes.data, ng, pfl, ld,
                                                             ctypes.c_void_p(d_out) if d_out else None, ctypes.c_void_p(d_outDot)))

    def flowIntegrateBwd(self, outBar, n: int, par, groups=None, level: int = 1, frozenTurb=False, useTurbOnly=False, ld=None, fill=0.0):
        """wbar (nRhs, ld) as wallIntegrateBwd, for the in- and outflow subfaces"""
        par, ng, fl, pfl, ldf, flags = self._flowArgs(par, groups, frozenTurb, useTurbOnly)
        ob = np.ascontiguousarray(outBar, dtype=np.float64).reshape(-1, max(ng, 1), capi.WALLINT_STRIDE)
        ld = int(n) if ld is None else int(ld)
        wbar = np.full((ob.shape[0], max(ld, 1)), float(fill))
        self._chk(self.lib.adflow_gpu_flow_integrate_bwd(level, flags, par.ctypes.data, ng, pfl, ldf, ob.ctypes.data, ob.shape[0],
                                                         wbar.ctypes.data, int(n), ld))
        return wbar

    def flowIntegrateBwdDev(self, outBar, d_wbar: int, n: int, ld: int, par, groups=None, level: int = 1, frozenTurb=False,
                            useTurbOnly=False):
        """the same into device vectors ld doubles apart (outBar stays a host array); honours set_async"""
        par, ng, fl, pfl, ldf, flags = self._flowArgs(par, groups, frozenTurb, useTurbOnly)
        ob = np.ascontiguousarray(outBar, dtype=np.float64).reshape(-1, max(ng, 1), capi.WALLINT_STRIDE)
        self._chk(self.lib.adflow_gpu_flow_integrate_bwd_dev(level, flags, par.ctypes.data, ng, pfl, ldf, ob.ctypes.data, ob.shape[0],
                                                             ctypes.c_void_p(d_wbar), int(n), int(ld)))

    def upload_coordinates(self, nn=1, level=1, sps=1):
        self._chk(self.lib.adflow_gpu_upload_coordinates(nn, level, sps))

    def update_geometry(self, level=1):
        """volume_block + metric_block + boundaryNormals on the device"""
        self._chk(self.lib.adflow_gpu_update_geometry(level))

    def comm_register_periodic(self, level, nLayers, periodic):
        """periodic: list of dicts rotMatrix (3,3), rotCenter (3), translation (3), block (n) int32, indices (n,3) int32 F-order"""
        arr = (capi.AdflowPeriodicData * max(len(periodic), 1))()
        keep = []
        for m, pd in enumerate(periodic):
            R = np.asfortranarray(pd["rotMatrix"], dtype=np.float64)
            for q in range(9):
                arr[m].rotMatrix[q] = float(R.ravel(order="F")[q])
            for q in range(3):
                arr[m].rotCenter[q] = float(pd["rotCenter"][q])
                arr[m].translation[q] = float(pd["translation"][q])
            blk = np.ascontiguousarray(pd["block"], np.int32)
            idx = np.asfortranarray(pd["indices"], np.int32)
            keep += [blk, idx]
            arr[m].nHalos = int(blk.size)
            arr[m].block = blk.ctypes.data
            arr[m].indices = idx.ctypes.data
        self._chk(self.lib.adflow_gpu_comm_register_periodic(level, nLayers, len(periodic), arr))

    def actuator_register(self, regions):
        """regions: list of dicts block (n) int32, cellIDs (3,n) int32 F-order, force (3), heat, volume, relaxStart, relaxEnd"""
        arr = (capi.AdflowActuatorRegion * max(len(regions), 1))()
        keep = []
        for m, r in enumerate(regions):
            blk = np.ascontiguousarray(r["block"], np.int32)
            ids = np.asfortranarray(r["cellIDs"], np.int32)
            keep += [blk, ids]
            arr[m].nCellIDs = int(blk.size)
            arr[m].block, arr[m].cellIDs = blk.ctypes.data, ids.ctypes.data
            for q in range(3):
                arr[m].force[q] = float(r["force"][q])
            arr[m].heat, arr[m].volume = float(r["heat"]), float(r["volume"])
            arr[m].relaxStart, arr[m].relaxEnd = float(r.get("relaxStart", -1.0)), float(r.get("relaxEnd", -1.0))
        self._chk(self.lib.adflow_gpu_actuator_register(len(regions), arr))

    def xhalo(self, level=1):
        """xhalo_block of every block of the level"""
        self._chk(self.lib.adflow_gpu_xhalo(level))

    def coarseOwnedCoordinates(self, coarseLevel):
        self._chk(self.lib.adflow_gpu_coarse_coordinates(coarseLevel))

    def exchangeCoor(self, level=1):
        self._chk(self.lib.adflow_gpu_exchange_coor(level))

    def applyAllBC(self, level=1, secondHalo=True):
        self._chk(self.lib.adflow_gpu_apply_all_bc(level, int(secondHalo)))

    def set_tuning(self, key: str, value: int):
        self._chk(self.lib.adflow_gpu_set_tuning(key.encode(), int(value)))

    def set_async(self, on: bool):
        """Entry points only enqueue on the library stream; order with sync()."""
        self._chk(self.lib.adflow_gpu_set_async(int(on)))

    def RungeKuttaSmoother(self, level=1):
        self._chk(self.lib.adflow_gpu_rk_smooth(level))

    def DADISmoother(self, level=1):
        self._chk(self.lib.adflow_gpu_dadi_smooth(level))

    def turbSolveDDADI(self, level=1):
        self._chk(self.lib.adflow_gpu_sa_solve(level))

    # ---- Newton-Krylov glue (nksolver.* of src/f2py/adflow.pyf:394-421) -----
    def setW(self, wVec: np.ndarray):
        assert wVec.dtype == np.float64 and wVec.flags["C_CONTIGUOUS"]
        self._chk(self.lib.adflow_gpu_set_w_vec(wVec.ctypes.data, wVec.size))

    def setRVec(self, n: int):
        """-> (rVec, sum flow^2, sum turb^2)"""
        r = np.zeros(n)
        s2 = np.zeros(2)
        self._chk(self.lib.adflow_gpu_get_r_vec(r.ctypes.data, n, s2.ctypes.data))
        return r, s2[0], s2[1]

    def getRes(self, n: int):
        r = np.zeros(n)
        self._chk(self.lib.adflow_gpu_get_res(r.ctypes.data, n))
        return r

    def FormFunction_mf(self, wVec: np.ndarray):
        """setW + blocketteRes + setRVec (NKSolvers.F90:437-461)."""
        assert wVec.dtype == np.float64 and wVec.flags["C_CONTIGUOUS"]
        r = np.zeros_like(wVec)
        self._chk(self.lib.adflow_gpu_nk_residual(wVec.ctypes.data, r.ctypes.data, wVec.size))
        return r

    def FormFunction_mf_dev(self, d_wVec: int, d_rVec: int, n: int):
        """the same on device pointers (two device vectors of n doubles)"""
        self._chk(self.lib.adflow_gpu_nk_residual_dev(ctypes.c_void_p(d_wVec), ctypes.c_void_p(d_rVec), int(n)))

    # ---- multigrid ----------------------------------------------------------
    def transferToCoarseGrid(self, level=1):
        self._chk(self.lib.adflow_gpu_transfer_to_coarse(level))

    def transferToFineGrid(self, level=1):
        self._chk(self.lib.adflow_gpu_transfer_to_fine(level))

    def executeMGCycle(self, cycling):
        c = np.ascontiguousarray(cycling, np.int32)
        self._chk(self.lib.adflow_gpu_mg_cycle(c.ctypes.data, c.size))

    # ---- halo exchange ------------------------------------------------------
    def comm_register(self, level: int, nLayers: int, cp):
        """commPatternCell_{1st,2nd}(level) + internalCell_{1st,2nd}(level)."""
        c = capi.comm_pattern_struct(cp)
        self._chk(self.lib.adflow_gpu_comm_register(level, nLayers, ctypes.byref(c)))

    def comm_init_single(self):
        """RCCL communicator of ONE rank (adflow_gpu_comm_unique_id + adflow_gpu_comm_init(0, 1, id)): what a multi-rank host does
        with the id broadcast over MPI / torch.distributed; enough for messages to the own rank (tuning comm_self)."""
        if getattr(self, "_comm_ready", False):
            return
        raw = (ctypes.c_char * 128)()
        self._chk(self.lib.adflow_gpu_comm_unique_id(raw))
        self._chk(self.lib.adflow_gpu_comm_init(0, 1, raw))
        self._comm_ready = True

    def comm_info(self):
        """(rank, nranks as given to adflow_gpu_comm_init; ncclCommCount, ncclCommUserRank as the communicator reports them, -1 before)"""
        v = [ctypes.c_int() for _ in range(4)]
        self._chk(self.lib.adflow_gpu_comm_info(*[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def whalo1(self, level, start, end, commPressure=True, commGamma=True, commViscous=True):
        self._chk(self.lib.adflow_gpu_halo_exchange(level, start, end, int(commPressure), int(commViscous), 1))

    def whalo2(self, level, start, end, commPressure=True, commGamma=True, commViscous=True):
        self._chk(self.lib.adflow_gpu_halo_exchange(level, start, end, int(commPressure), int(commViscous), 2))

    def res_norms(self, level=1, n=5):
        out = np.zeros(n)
        self._chk(self.lib.adflow_gpu_res_norms(level, out.ctypes.data, n))
        return out

    # ---- instrumentation ----------------------------------------------------
    def event_record(self, slot: int):
        self._chk(self.lib.adflow_gpu_event_record(slot))

    def event_elapsed_ms(self, a: int, b: int) -> float:
        ms = ctypes.c_double()
        self._chk(self.lib.adflow_gpu_event_elapsed_ms(a, b, ctypes.byref(ms)))
        return ms.value

    def march_stats(self, level: int = 1):
        out = (ctypes.c_double * 4)()
        self._chk(self.lib.adflow_gpu_march_stats(level, out, 4))
        return {"sa_march": out[0], "visc_gf": out[1], "tile_march": out[2]}

    def sync(self):
        self._chk(self.lib.adflow_gpu_sync())
