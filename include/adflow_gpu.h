/*
 * adflow_gpu.h — C-ABI of the MI355X residual / smoother engine.
 *
 * This is the drop-in boundary of SURVEY.md §8(b).  The reference has no
 * plugin registry: its hot path is a set of Fortran module procedures that act
 * on module-global block pointers.  A maintainer keeps all host Fortran and
 * replaces the BODIES of the shell routines listed next to each entry point by
 * a call through an ISO_C_BINDING interface to the function below
 * (INTEGRATION.md shows the Fortran side; adflow_amd/fortran/adflow_gpu_shim.F90
 * is that interface module).
 *
 * Conventions
 *  - plain C types only; every function returns 0 on success, nonzero on error
 *    (adflow_gpu_last_error() gives the text; the Fortran shim forwards it to
 *    utils::terminate, src/utils/utils.F90:501).
 *  - host arrays are the reference's own Fortran arrays, column-major, with the
 *    bounds the reference allocates (SURVEY.md §8(a) row "T"); the library
 *    NEVER takes ownership — it only keeps device mirrors.
 *  - (nn, level, sps) identify a block exactly like flowDoms(nn,level,sps)
 *    (src/modules/block.F90:760-775); all three are 1-based.
 *  - reals are double (realType, src/modules/precision.F90:77-81), integers
 *    int32 (intType), porosities int8 (porType, precision.F90:110-111).
 *  - single host thread per process; all work is issued on one HIP stream per
 *    process and every entry point is synchronous on return unless stated.
 */
#ifndef ADFLOW_GPU_H
#define ADFLOW_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enumerations: values of src/modules/constants.F90 */
enum { ADFLOW_EULER = 1, ADFLOW_NS = 2, ADFLOW_RANS = 3 };
enum { ADFLOW_DISS_SCALAR = 1, ADFLOW_DISS_MATRIX = 2, ADFLOW_UPWIND = 9 };
enum { ADFLOW_LIM_FIRST_ORDER = 1, ADFLOW_LIM_NONE = 2, ADFLOW_LIM_VANALBADA = 3, ADFLOW_LIM_MINMOD = 4 };
enum { ADFLOW_RUNGE_KUTTA = 1, ADFLOW_DADI = 2 };
enum { ADFLOW_TURBPROD_STRAIN = 1, ADFLOW_TURBPROD_VORTICITY = 2 };
enum { ADFLOW_RESAVG_NEVER = 0, ADFLOW_RESAVG_ALWAYS = 1, ADFLOW_RESAVG_ALTERNATE = 2 };

#define ADFLOW_MAX_RK_STAGES 8

/* host hook type: see adflow_gpu_set_bc_callback */
typedef void (*adflow_bc_callback)(int level, int secondHalo);

/* boundary subfaces: BCType and BCFaceID values of src/modules/constants.F90:257-297 */
enum {
    ADFLOW_BC_SYMM = -1, ADFLOW_BC_SYMM_POLAR = -2, ADFLOW_BC_NSWALL_ADIABATIC = -3, ADFLOW_BC_NSWALL_ISOTHERMAL = -4,
    ADFLOW_BC_EULERWALL = -5, ADFLOW_BC_FARFIELD = -6, ADFLOW_BC_SUPERSONIC_INFLOW = -7, ADFLOW_BC_SUBSONIC_INFLOW = -8,
    ADFLOW_BC_SUPERSONIC_OUTFLOW = -9, ADFLOW_BC_SUBSONIC_OUTFLOW = -10, ADFLOW_BC_MASSBLEED_OUTFLOW = -12,
    ADFLOW_BC_EXTRAP = -15
};
enum { ADFLOW_INLET_TOTAL_CONDITIONS = 1, ADFLOW_INLET_MASS_FLOW = 2 };   /* BCData%subsonicInletTreatment, constants.F90:237 */
enum { ADFLOW_IMIN = 1, ADFLOW_IMAX = 2, ADFLOW_JMIN = 3, ADFLOW_JMAX = 4, ADFLOW_KMIN = 5, ADFLOW_KMAX = 6 };
enum { ADFLOW_WALLBC_CONSTANT = 1, ADFLOW_WALLBC_LINEAR = 2, ADFLOW_WALLBC_QUADRATIC = 3, ADFLOW_WALLBC_NORMAL_MOMENTUM = 4 };

/* One boundary subface of a block: flowDoms(nn,level,sps)%BCType(mm), %BCFaceID(mm) and the
 * members of %BCData(mm) the flow boundary conditions read (block.F90 BCDataType).  Every array
 * has the bounds (icBeg:icEnd, jcBeg:jcEnd [,3]) of the reference, Fortran order; NULL where the
 * boundary type does not use it (rface NULL = zero grid velocity). */
typedef struct adflow_bc_subface {
    int32_t bcType, faceID;
    int32_t icBeg, icEnd, jcBeg, jcEnd;
    int32_t subsonicInletTreatment;   /* SubsonicInflow: 1 total conditions, 2 mass flow                 */
    int32_t reserved;
    const double* norm;       /* unit outward normal, 3 components                                       */
    const double* rface;      /* normal grid velocity (EulerWall, farField)                              */
    const double* uSlip;      /* wall velocity, 3 components (NSWall*)                                   */
    const double* TNS_Wall;   /* wall temperature (NSWallIsothermal)                                     */
    const double* rho;        /* prescribed state (SupersonicInflow; SubsonicInflow with mass flow): rho, velx, vely, velz */
    const double* velx;
    const double* vely;
    const double* velz;
    const double* ps;         /* static pressure (SupersonicInflow, SubsonicOutflow, MassBleedOutflow)   */
    const double* ptInlet;    /* SubsonicInflow with total conditions: total pressure, temperature, enthalpy, */
    const double* ttInlet;    /* unit flow direction                                                     */
    const double* htInlet;
    const double* flowXdirInlet;
    const double* flowYdirInlet;
    const double* flowZdirInlet;
    const double* turbInlet;  /* prescribed turbulence variable(s) of inflow subfaces (RANS), (:,:,nt1:nt2) */
    double symNorm[3];        /* BCData%symNorm: the (constant) normal of a symmetry plane, read by xhalo_block */
} adflow_bc_subface;

/* Options: snapshot of the Fortran module variables the hot path reads.
 * Refreshed by the shim at every entry (Python may assign them between calls,
 * adflow/pyADflow.py:5463-5630).  Field names are the reference's. */
typedef struct adflow_opts {
    /* inputPhysics (src/modules/inputParam.F90:507-635) */
    int32_t equations, turbModel, turbProd;
    int32_t useQCR, useRotationSA, useft2SA;
    /* inputDiscretization (inputParam.F90:1-97) */
    int32_t spaceDiscr, spaceDiscrCoarse, limiter, orderTurb;
    int32_t dirScaling;
    /* inputIteration (inputParam.F90:183-299) */
    int32_t smoother, nRKStages, resAveraging, nSubiterations, nSubIterTurb;
    /* iteration (src/modules/iteration.f90) */
    int32_t groundLevel;
    int32_t turbRelax;        /* inputIteration: 1 explicit, 2 implicit (default for SA, inputParamRoutines.F90:3402) */
    /* inputDiscretization: boundary treatment (constants.F90:170-178): 1 constant, 2 linear, 4 normal momentum;
     * outflowTreatment 1 constant, 2 linear extrapolation */
    int32_t eulerWallBCTreatment, viscWallBCTreatment, outflowTreatment;
    int32_t hScalingInlet;            /* inputDiscretization: total-enthalpy scaling of the subsonic-inflow Riemann invariant */
    /* features of the reference this library does NOT implement, as a bit mask the host fills from its option modules:
     * 1 equationMode /= steady (unsteady / time spectral), 2 cpModel /= cpConstant, 4 wall functions, 8 overset blocks present.
     * adflow_gpu_set_options refuses a non-zero mask instead of silently returning steady, constant-gamma, 1-to-1 results. */
    int32_t unsupported;
    int32_t lowSpeedPreconditioner;   /* inputDiscretization: residual_block's 5x5 low-Mach transform (residuals.F90:172-331) + the 0.8 RK step factor (smoothers.F90:202) */
    /* iteration::exchangePressureEarly (iteration.f90:44-53; set by solvers.F90:35-39,140-144 = eulerWallBcTreatment == normalMomentum
     * .and. EulerWallsPresent(), a reduction over ALL processes): pressure-only whalo1 before applyAllBC in every smoother stage
     * and in transferToFineGrid (smoothers.F90:363,674, multiGrid.F90:602) */
    int32_t exchangePressureEarly;
    int32_t reserved_i;
    double gammaConstant, prandtl, prandtlTurb;
    double SSuthDim, muSuthDim, TSuthDim;
    double SAKappa, SAcb1, SAcb2, SAsigma, SAcv1, SAcw1, SAcw2, SAcw3, SAct1, SAct2, SAct3, SAct4, SAcrot;
    double vis2, vis4, vis2Coarse, adis, acousticScaleFactor, kappaCoef;
    double cfl, cflCoarse, cflLimit, fcoll, smoop, alfaTurb, betaTurb, turbResScale;
    double etaRK[ADFLOW_MAX_RK_STAGES], cdisRK[ADFLOW_MAX_RK_STAGES];
    /* flowVarRefState (src/modules/flowVarRefState.F90) */
    double gammaInf, pInf, pInfCorr, rhoInf, uInf, RGas, muInf, muRef, TRef, timeRef;
    double wInf[10];
    double sigma;             /* inputDiscretization: lumped-dissipation coefficient of the approximate residual */
    double pRef, uRef, LRef;  /* flowVarRefState: scales of the actuator-region source terms (residuals.F90:370-385) */
    double ordersConverged;   /* iteration: relaxation of the actuator source between relaxStart and relaxEnd */
    double reserved_d[3];
} adflow_opts;

/* Host arrays of one block, flowDoms(nn,level,sps)%... .  NULL = not present
 * (e.g. rev for Euler).  Bounds in comments are the reference's allocation. */
typedef struct adflow_block_desc {
    int32_t nx, ny, nz;       /* owned cells: il=nx+1, ie=nx+2, ib=nx+3 (block.F90:363-390) */
    int32_t nw;               /* 5, or 6 with Spalart-Allmaras */
    int32_t rightHanded;      /* blockType%rightHanded */
    int32_t reserved;
    /* state (initializeFlow.F90:457-529) */
    double *w;                /* (0:ib,0:jb,0:kb,1:nw)  rho,u,v,w,rhoE[,nuTilde] */
    double *p, *gamma;        /* (0:ib,0:jb,0:kb) */
    double *rlv, *rev;        /* (0:ib,0:jb,0:kb) */
    /* geometry */
    double *x;                /* (0:ie,0:je,0:ke,3)  partitioning.F90:1761 */
    double *sI, *sJ, *sK;     /* (0:ie,1:je,1:ke,3) (1:ie,0:je,1:ke,3) (1:ie,1:je,0:ke,3) */
    double *vol, *volRef;     /* (0:ib,0:jb,0:kb) */
    double *d2Wall;           /* (2:il,2:jl,2:kl)  wallDistance.F90:503 */
    int8_t *porI, *porJ, *porK; /* (1:il,2:jl,2:kl) (2:il,1:jl,2:kl) (2:il,2:jl,1:kl) preprocessingAPI.F90:567 */
    int32_t *iblank;          /* (0:ib,0:jb,0:kb) */
    /* residual / work arrays the host may want back (utils.F90:3969-3974) */
    double *dw;               /* (0:ib,0:jb,0:kb,1:nw) */
    double *fw;               /* (0:ib,0:jb,0:kb,1:5) */
    double *dtl, *radI, *radJ, *radK; /* (1:ie,1:je,1:ke) */
    /* multigrid work (coarse levels, initializeFlow.F90:746-748) */
    double *w1, *p1, *wr;     /* (1:ie,1:je,1:ke,1:5) (1:ie,1:je,1:ke) (2:il,2:jl,2:kl,1:5) */
    /* multigrid transfer maps (src/preprocessing/coarseUtils.F90:254-262), NULL when absent.
     * On a COARSE block: the two fine cells of each coarse cell and the restriction weights */
    int32_t *mgIFine, *mgJFine, *mgKFine;       /* (1:ie,2) (1:je,2) (1:ke,2) */
    double *mgIWeight, *mgJWeight, *mgKWeight;  /* (2:il) (2:jl) (2:kl) */
    /* on a FINE block: nearest and next-nearest coarse cell of each fine cell */
    int32_t *mgICoarse, *mgJCoarse, *mgKCoarse; /* (2:il,2) (2:jl,2) (2:kl,2) */
    /* moving blocks (rotating frame / ALE, block.F90 sFaceI/J/K, addGridVelocities, blockIsMoving): dot product of the
     * face velocity with the face normal; NULL / 0 for a block at rest.  rotRate = cgnsDoms(nbkGlobal)%rotRate, used by
     * the rotational source of inviscidCentralFlux (fluxes.F90:372-397) when blockIsMoving in steady mode */
    double *sFaceI, *sFaceJ, *sFaceK;           /* (0:ie,1:je,1:ke) (1:ie,0:je,1:ke) (1:ie,1:je,0:ke) */
    double rotRate[3];
    int32_t addGridVelocities, blockIsMoving;
} adflow_block_desc;

/* 1-to-1 halo communication pattern of one level and one halo depth: the
 * reference's internalCell_{1st,2nd}(level) and commPatternCell_{1st,2nd}(level)
 * (src/modules/communication.F90 internalCommType / commType), flattened.  Cell
 * indices are the values the reference stores (actual cell indices 0..ib; its
 * "+1" at use, haloExchange.F90:605-607, only undoes a pointer rebasing).
 * Index arrays are column-major (n,3) like the Fortran ones; block ids are the
 * local block numbers nn (1-based).  Entry order inside a message must match on
 * sender and receiver, which the reference's preprocessing guarantees. */
typedef struct adflow_comm_pattern {
    int32_t ncopy;                       /* internal%ncopy: same-process copies */
    const int32_t *donorBlock, *donorIndices;   /* (ncopy), (ncopy,3) */
    const int32_t *haloBlock, *haloIndices;     /* (ncopy), (ncopy,3) */
    int32_t nProcSend;                   /* commPattern%nProcSend */
    const int32_t *sendProc;             /* (nProcSend) ranks */
    const int32_t *nsendCum;             /* (0:nProcSend) cumulative cell counts, nsendCum[0] = 0 */
    const int32_t *sendBlock, *sendIndices;     /* (nsendCum[nProcSend]), (..,3): sendList(i)%block / %indices concatenated */
    int32_t nProcRecv;
    const int32_t *recvProc;
    const int32_t *nrecvCum;
    const int32_t *recvBlock, *recvIndices;
} adflow_comm_pattern;

/* identifiers for adflow_gpu_download_array / adflow_gpu_upload_array */
enum {
    ADFLOW_ARR_W = 1, ADFLOW_ARR_P, ADFLOW_ARR_GAMMA, ADFLOW_ARR_RLV, ADFLOW_ARR_REV,
    ADFLOW_ARR_DW, ADFLOW_ARR_FW, ADFLOW_ARR_DTL, ADFLOW_ARR_RADI, ADFLOW_ARR_RADJ, ADFLOW_ARR_RADK,
    ADFLOW_ARR_AA, ADFLOW_ARR_NODAL_GRADS, ADFLOW_ARR_WN, ADFLOW_ARR_PN, ADFLOW_ARR_W1, ADFLOW_ARR_P1,
    ADFLOW_ARR_WR, ADFLOW_ARR_VOL, ADFLOW_ARR_SI, ADFLOW_ARR_SJ, ADFLOW_ARR_SK, ADFLOW_ARR_X,
    ADFLOW_ARR_D2WALL                  /* d2Wall(2:il,2:jl,2:kl) */
};

/* flags of adflow_gpu_block_res: the logical arguments of blockette::blocketteRes
 * (src/NKSolver/blockette.F90:70-120) */
enum {
    ADFLOW_RES_UPDATE_INTERMED = 1u,   /* also store dtl, radI/J/K.  WITHOUT it the spectral radii and dtl are not outputs of the call
                                          (as in blocketteResCore, which keeps them in tile-private arrays): for matrix dissipation
                                          and Roe upwind they are not formed at all, and ADFLOW_ARR_RADI/J/K, ADFLOW_ARR_DTL on the
                                          device are UNDEFINED afterwards (adflow_gpu_time_step or a call with this flag refreshes
                                          them; the smoothers call the time step themselves) */
    ADFLOW_RES_FLOW = 2u,              /* useFlowRes  */
    ADFLOW_RES_TURB = 4u,              /* useTurbRes  */
    /* the part of blocketteRes in front of the core (blockette.F90:195-246): */
    ADFLOW_RES_CLOSURES = 8u,          /* computePressureSimple + laminar/eddy viscosity, owned cells */
    ADFLOW_RES_HALO = 16u,             /* boundary-condition hook + whalo2(1, lStart, lEnd, T,T,T) */
    /* approximate residual of the preconditioner assembly (blockette.F90:755-852, fluxes.F90:3487-4975): */
    ADFLOW_RES_DISS_APPROX = 32u,      /* useDissApprox: inviscidDissFluxScalarApprox / MatrixApprox (lumped 2nd-difference
                                          dissipation with the FROZEN sensor of adflow_gpu_reference_shock_sensor) */
    ADFLOW_RES_VISC_APPROX = 64u,      /* useViscApprox: viscousFluxApprox (thin-layer normal differences) */
    /* with DISS_APPROX and the Roe upwind scheme the two residual cores of the reference differ: blocketteResCore (useBlockettes = T,
     * the default) calls inviscidUpwindFlux(.False.) = first-order reconstruction (blockette.F90:643), blockResCore keeps the
     * limiter (:827).  The host passes this flag when inputDiscretization::useBlockettes is set. */
    ADFLOW_RES_UPWIND_FIRST_ORDER = 128u,
    /* (256u and 512u are ADFLOW_ANK_COUPLED and ADFLOW_ANK_TURB, which share the flag word of the adflow_gpu_ank_* entries) */
    /* inputDiscretization::approxSA (set by ANKStep:3848-3852, FormJacobianANK:1978, FormJacobianANKTurb:2364 while
     * totalR > ANK_secondOrdSwitchTol totalR0): term1 of the SA source is zero (sa.F90:296, blockette.F90:1016, sa_d.f90:454/654) */
    ADFLOW_RES_APPROX_SA = 1024u,
    /* orderTurb = firstOrder for this call only (ANKTurbSolveKSP:3411-3412, ANKStep:3855-3856); the option is restored on return */
    ADFLOW_RES_TURB_FIRST_ORDER = 2048u
};

/* ---- lifetime ---------------------------------------------------------- */
int adflow_gpu_init(int device_ordinal);
int adflow_gpu_finalize(void);
const char* adflow_gpu_last_error(void);
int adflow_gpu_device_name(char* buf, int len);

/* ---- multi-GPU (RCCL over xGMI) replaces the MPI path of
 *      src/utils/haloExchange.F90:553-719 ------------------------------------ */
int adflow_gpu_comm_unique_id(void* id128);                       /* rank 0: create id (128 bytes) */
int adflow_gpu_comm_init(int rank, int nranks, const void* id128); /* all ranks */
/* What the communicator itself reports (ncclCommCount / ncclCommUserRank; -1 / -1 before adflow_gpu_comm_init) beside the rank and
 * size the library was given: lets a launcher check that every rank joined ONE communicator of the expected size before the first
 * exchange (the reference's myID / nProc of communication.F90 come from MPI_Comm_rank / _size the same way). */
int adflow_gpu_comm_info(int* rank, int* nranks, int* commCount, int* commUserRank);

/* ---- data model -------------------------------------------------------- */
int adflow_gpu_block_register(int nn, int level, int sps, const adflow_block_desc* d);
/* free the device mirrors of one block / of every block (utils::releaseMemoryPart1/2,
 * src/utils/utils.F90:4253,4732); host arrays are untouched */
int adflow_gpu_block_release(int nn, int level, int sps);
int adflow_gpu_release_all(void);
int adflow_gpu_upload_geometry(int nn, int level, int sps);   /* x,sI,sJ,sK,vol,volRef,d2Wall,por*,iblank */
/* Mesh warping ("next" row 3 of SURVEY.md 8f): upload the node coordinates only, then derive cell volumes, face
 * normals and the unit normals of the registered boundary subfaces on the device = volume_block + metric_block +
 * boundaryNormals (src/adjoint/adjointExtra.F90:5-364), the `useSpatial` branch of blocketteRes (blockette.F90:203-211) */
int adflow_gpu_upload_coordinates(int nn, int level, int sps);
int adflow_gpu_update_geometry(int level);
/* wallDistance::updateWallDistancesQuickly (src/wallDistance/wallDistance.F90:36-120), called by the `useSpatial` branch for RANS
 * with useApproxWallDistance (blockette.F90:207-209): d2Wall of the owned cells = | cell centre - closest wall point |, the wall
 * point re-formed from the association the host found once (determineWallAssociation, :1663-2002) and the current surface
 * coordinates.  register: flowDoms(nn,level,sps)%surfNodeIndices(4,2:il,2:jl,2:kl) (1-based numbers into xSurf, first = 0: no wall
 * within reach, d2Wall = large) and %uv(2,2:il,2:jl,2:kl).  update: xSurf = the scattered surface-node vector of updateXSurf
 * (:2004-2051), n = 3 x nodes; runs after adflow_gpu_update_geometry's coordinates are in place */
int adflow_gpu_wall_distance_register(int nn, int level, int sps, const int32_t* surfNodeIndices, const double* uv);
int adflow_gpu_update_wall_distances(int level, const double* xSurf, int64_t n);
/* Halo node coordinates after the owned nodes moved, the two steps that precede volume / metric in the `useSpatial`
 * branch of blocketteRes (blockette.F90:181-187):
 *   adflow_gpu_xhalo          adjointExtra::xhalo_block (adjointExtra.F90:365-599) of every block of the level: linear
 *                             extrapolation of the halo nodes 0 / ie, je, ke, then the mirror image in symmetry planes
 *                             (subfaces of kind symm with their BCData%symNorm);
 *   adflow_gpu_exchange_coor  haloExchange::exchangeCoor (haloExchange.F90:2456-2640): halo nodes of 1-to-1 interfaces
 *                             from the neighbours' interior nodes, using the NODE pattern commPatternNode_1st(level) /
 *                             internalNode_1st(level) registered with adflow_gpu_comm_register(level, 0, pattern)
 *                             (same-GPU copies + RCCL send/recv; periodic transformations as registered with
 *                             adflow_gpu_comm_register_periodic). */
int adflow_gpu_xhalo(int level);
/* coarseUtils::coarseOwnedCoordinates(coarseLevel) (coarseUtils.F90:780-858): the owned nodes of the coarse blocks from
 * the level above, through the registered mgI/J/KFine maps.  updateCoordinatesAllLevels / updateMetricsAllLevels
 * (preprocessingAPI.F90:3945-4017) on the device = for every coarse level: this, adflow_gpu_xhalo,
 * adflow_gpu_exchange_coor, adflow_gpu_update_geometry. */
int adflow_gpu_coarse_coordinates(int coarseLevel);
int adflow_gpu_exchange_coor(int level);
int adflow_gpu_upload_state(int nn, int level, int sps);      /* w,p,gamma,rlv,rev incl. both halo layers */
int adflow_gpu_download_state(int nn, int level, int sps);
int adflow_gpu_download_residual(int nn, int level, int sps); /* dw -> desc.dw */
int adflow_gpu_download_array(int nn, int level, int sps, int which, double* host);
int adflow_gpu_upload_array(int nn, int level, int sps, int which, const double* host);
int adflow_gpu_set_options(const adflow_opts* o);

/* ---- the hot path; each acts on ALL registered blocks of `level`, like the
 *      reference's shell loops over nDom -------------------------------------- */
/* solverUtils::timeStep (src/solver/solverUtils.F90:4-41, block body :43-356) */
int adflow_gpu_time_step(int level, int onlyRadii);
/* residuals::initres (src/solver/residuals.F90:964-1026, block body :427-955), 1-based var range */
int adflow_gpu_initres(int level, int varStart, int varEnd);
/* residuals::residual (src/solver/residuals.F90:1028-1060, block body :4-346);
 * rkStage selects rFil = cdisRK(rkStage+1) for the Runge-Kutta smoother */
int adflow_gpu_residual(int level, int rkStage);
/* blockette::blocketteRes main loop (src/NKSolver/blockette.F90:266-283):
 * timeStep + initres + [SA] + inviscid + [viscous] + dw=(dw+fw)*iblank, rFil=1 */
int adflow_gpu_block_res(int level, unsigned flags);
/* adjointUtils::referenceShockSensor (src/adjoint/adjointUtils.F90:1909-1969): freeze the shock sensor of every
 * level-1 block at the current state (pressure for Euler / matrix dissipation, entropy p/rho^gamma otherwise) for
 * the following ADFLOW_RES_DISS_APPROX evaluations */
int adflow_gpu_reference_shock_sensor(int level);
/* smoothers::RungeKuttaSmoother / DADISmoother (src/solver/smoothers.F90:4,383) */
int adflow_gpu_rk_smooth(int level);
int adflow_gpu_dadi_smooth(int level);
/* turbAPI::turbSolveDDADI for Spalart-Allmaras (src/turbulence/turbAPI.F90:4-95, sa.F90:16-86,717-1268):
 * nSubIterTurb x [SA residual + central jacobian, DDADI line solves j,i,k, update of
 * nuTilde and rev, turbulent-BC hook, whalo2(nt1:nt2)] */
int adflow_gpu_sa_solve(int level);
int adflow_gpu_set_turb_bc_callback(adflow_bc_callback fn);   /* applyAllTurbBCThisBlock stays on the host */
/* multigrid::transferToCoarseGrid (src/solver/multiGrid.F90:5-324): residual on `level`,
 * volume-weighted restriction to level+1, coarse residual, forcing term wr */
int adflow_gpu_transfer_to_coarse(int level);
/* multigrid::transferToFineGrid(.true.) (multiGrid.F90:326-652): prolongation of the
 * corrections of level+1 to `level`, state update, halo exchange */
int adflow_gpu_transfer_to_fine(int level);
/* multigrid::executeMGCycle (multiGrid.F90:825-955): `cycling` as produced by
 * setCycleStrategy (:957-1030): -1 prolongate, 0 smooth, +1 restrict; ends with the
 * turbSolveDDADI (RANS) and the ground-level time step + residual. */
int adflow_gpu_mg_cycle(const int32_t* cycling, int nStepsCycling);
/* register the 1-to-1 pattern of (level, nLayers = 1 | 2); lists are copied */
int adflow_gpu_comm_register(int level, int nLayers, const adflow_comm_pattern* p);
/* Periodic transformations of a registered pattern: the periodicData(:) of internalCell_*(level) AND commPatternCell_*(level)
 * (communication.F90 periodicDataType) concatenated - they address disjoint halos.  Applied on the receiving side after the
 * exchange: velocities of the listed halo cells rotated by rotMatrix when the exchanged range covers ivx..ivz
 * (correctPeriodicVelocity, haloExchange.F90:456-551); for the node pattern (nLayers = 0) the halo node coordinates become
 * rotMatrix (x - rotCenter) + translation + rotCenter (correctPeriodicCoor, haloExchange.F90:2644-2712).
 * Call after adflow_gpu_comm_register of the same (level, nLayers); nPeriodic = 0 removes them. */
typedef struct adflow_periodic_data {
    double rotMatrix[9];            /* (3,3) column-major, as stored */
    double rotCenter[3], translation[3];
    int32_t nHalos, reserved;
    const int32_t *block, *indices; /* (nHalos), (nHalos,3) column-major */
} adflow_periodic_data;
int adflow_gpu_comm_register_periodic(int level, int nLayers, int nPeriodic, const adflow_periodic_data* pd);
/* haloExchange::whalo1 (nLayers=1) / whalo2 (nLayers=2) (src/utils/haloExchange.F90:5,109):
 * w(varStart:varEnd) [+ p] [+ rlv, rev when viscous / eddy model]; 1-based variable range;
 * same-process copies on the device, other ranks through RCCL send/recv */
int adflow_gpu_halo_exchange(int level, int varStart, int varEnd, int commPressure, int commVisc, int nLayers);
/* split form of the inter-process part, for a caller-owned transport (used by the
 * CPU multi-process tests; the product path is adflow_gpu_halo_exchange):
 * pack the message for send slot `islot` (0-based) into `buf` (host or device
 * memory of nvar*count doubles, variable-major); unpack recv slot `islot` from `buf`;
 * *_count return the number of cells of the slot and the peer rank */
int adflow_gpu_halo_slot_info(int level, int nLayers, int isSend, int islot, int* peer, int* count);
int adflow_gpu_halo_pack(int level, int nLayers, int islot, int varStart, int varEnd, int commPressure, int commVisc, double* buf);
int adflow_gpu_halo_unpack(int level, int nLayers, int islot, int varStart, int varEnd, int commPressure, int commVisc, const double* buf);
int adflow_gpu_halo_local_copy(int level, int nLayers, int varStart, int varEnd, int commPressure, int commVisc);
/* host hook called between the state update and the halo exchange of every
 * smoother stage, where the reference applies boundary conditions
 * (applyAllBC, smoothers.F90:369,680).  NULL (default) = no physical boundaries. */
int adflow_gpu_set_bc_callback(adflow_bc_callback fn);
/* Boundary conditions on the device ("next" row 1 of SURVEY.md §8f).
 * adflow_gpu_bc_register copies the subfaces of one block (the first nViscBocos are the viscous
 * walls, as in the reference) to the device; adflow_gpu_apply_all_bc is BCRoutines::applyAllBC
 * (src/solver/BCRoutines.F90:15-221: symm -> adiabatic wall -> isothermal wall -> farfield ->
 * extrap / supersonic outflow -> Euler wall -> supersonic inflow, subfaces in index order inside
 * each kind, computeEtot + extrapolate2ndHalo as there) for every registered block of the level.
 * Once a level has registered subfaces the smoothers, the multigrid transfers and the NK residual
 * apply them on the device at the points where the reference calls applyAllBC; the host callback
 * (if any) still runs afterwards for kinds that are not implemented here (bleed inflow, mDot / thrust,
 * domain interfaces, sliding interfaces; normal-momentum Euler wall: registration of those returns an error). */
int adflow_gpu_bc_register(int nn, int level, int sps, int nBocos, int nViscBocos, const adflow_bc_subface* faces);
int adflow_gpu_apply_all_bc(int level, int secondHalo);
/* viscSubface(mm)%tau(:,:,1:6) and %q(:,:,1:3) of viscous subface mm (1-based, mm <= nViscBocos): the wall stress tensor and
 * heat flux that viscousFlux stores when rkStage == 0 on the ground level (storeWallTensor, fluxes.F90:2586-2592, 2861-2892)
 * and that the host's force integration reads (surfaceIntegrations.F90:718).  The arrays cover the owned face cells
 * inBeg+1:inEnd x jnBeg+1:jnEnd as allocated by viscSubfaceInfo (preprocessingAPI.F90:2520-2541); either may be NULL.
 * The device stores them after every such residual evaluation (adflow_gpu_residual with rkStage 0, the D-ADI smoother,
 * the multigrid cycle's closing residual, adflow_gpu_block_res). */
int adflow_gpu_download_wall_stress(int nn, int level, int sps, int mm, double* tau, double* q);
/* Surface integration on the device: surfaceIntegrations::wallIntegrationFace (surfaceIntegrations.F90:406-881) over the wall
 * subfaces (EulerWall, NSWallAdiabatic, NSWallIsoThermal) of every block of a level, as integrateSurfaces calls it per family
 * group, and the family minimum of Cp of computeCpMinFamily (:1363-1437).
 *
 * adflow_gpu_bc_set_families: BCData(mm)%famID of the nBocos registered subfaces of a block (nBocos as given to
 * adflow_gpu_bc_register) and, optionally, BCData(mm)%iblank over the OWNED face cells inBeg+1:inEnd x jnBeg+1:jnEnd (the bounds of
 * adflow_gpu_download_wall_stress), Fortran order, int8; iblank NULL, or NULL for a subface, means all ones (overset is refused by
 * adflow_gpu_set_options, so 1 is what the reference holds).  A block whose families were never set has family 0 everywhere;
 * adflow_gpu_bc_register replaces the subfaces and with them their families and blanking.
 *
 * adflow_gpu_wall_integrate[_dev]: par = ADFLOW_WALLINT_NPAR doubles at the indices below, named after the reference's variables
 * (inputPhysics, inputCostFunctions); pInf, pRef, gammaInf, LRef and equations come from adflow_gpu_set_options.  famLists = the
 * reference's famLists array: nGroups rows of ldFam entries, column-major (entry j of group g at g + nGroups j), first entry the
 * number of families that follow; nGroups = 0 (famLists unused) = one group holding every wall subface.  out = ADFLOW_WALLINT_STRIDE
 * doubles per group: entries 0..62 are this process's localValues(1:63) at the reference's indices (constants.F90:454-500) -- iFp,
 * iFv, iMp, iMv, iSepSensor, iSepAvg, iCavitation, iyPlus, iAxisMoment, iCpMin (the KS sum), iCoForceX/Y/Z; every other slot is
 * zero -- which the host adds into localVal before its own mpi_allreduce and getCostFunctions; entry 63 is the minimum of Cp over
 * the faces of the group with iblank = 1 (start value 10000).  A host that wants the cavitation KS sum calls once, reduces entry
 * 63 over its ranks, sets ADFLOW_WALLINT_CPMIN_FAMILY and calls again.  The entry reads what is on the device -- the halos as the last
 * boundary-condition pass left them, tau as the last storing evaluation left it (see adflow_gpu_download_wall_stress) -- evaluates
 * nothing itself and changes neither state nor residual.  Deterministic: two-pass sums in a fixed order, no atomics.  The _dev form
 * takes a device pointer for out and honours adflow_gpu_set_async; it waits for the queue only when the family lists differ from those of
 * the previous call on the level (the membership table is then replaced).
 * Errors (nothing is launched or allocated): a level without registered boundary subfaces; a viscous wall subface whose stress was
 * never stored; nGroups < 0; a family count above ldFam - 1; MachCoef <= 0; a moment axis of zero length.
 *
 * adflow_gpu_download_wall_forces: BCData(mm)%Fp(:,:,3), %Fv(:,:,3), %area of subface mm (1-based, any wall subface of the block)
 * as the last integration of the level left them, over the owned face cells; unblanked, Fv zero on an Euler wall; any pointer may
 * be NULL.
 *
 * Buffers: 7 doubles per owned wall face, the partial sums and the membership table are allocated at the first integration of a
 * level (a process that never integrates holds the bytes it held).  adflow_gpu_release_workspace FREES them and counts them in
 * its bytes (the next integration allocates them again); adflow_gpu_bc_register, adflow_gpu_bc_set_families,
 * adflow_gpu_block_release and adflow_gpu_release_all free them too.
 * Not here (the in- and outflow faces: adflow_gpu_flow_integrate below): zippers, user surfaces, actuator regions;
 * computeSepSensorKs and CpError2 (they need a family maximum and CpTarget; iSepSensorKs, iSepSensorArea, iSepSensorKsArea and
 * iCpError2 are zero); getCostFunctions, which stays on the host; the derivative seeds of master_d / master_b other than those
 * of the state (below).
 *
 * ---- derivatives of the integration with respect to the state -----------------------------------------------------------------------
 * What master_d adds to funcsDot and master_b to wbar for the wall subfaces (wallIntegrationFace_d / _b behind the front of
 * block_res_state_d), on the ground level.  Vectors are in the PETSc layout of adflow_gpu_jacfree_mult; flags is the ADFLOW_JAC_* set
 * that selects the state range: 0 (all nw variables), ADFLOW_JAC_FROZEN_TURB (the five flow variables) or ADFLOW_JAC_TURB_ONLY.
 * par, nGroups, famLists, ldFam: as for adflow_gpu_wall_integrate.  Both entries evaluate the front of the residual on dual numbers
 * themselves -- closures with halos, turbulence boundary conditions where the flags keep them, flow boundary conditions, the nodal
 * gradients of the wall node planes, the wall stress, the face terms -- at the state on the device, and run no time step and no flux
 * kernel; the plain state, its halos, the stored wall stress and the per-face Fp / Fv / area are not written, and the halos of
 * the state are read as they are on the device, as the integration reads them (no 2-layer exchange of the state).  Entries 17 (yplusMax) and 63 (the minimum of Cp) are not differentiated,
 * as in the reference: their derivative is zero.
 *
 * adflow_gpu_wall_integrate_fwd[_dev]: outDot (nGroups x ADFLOW_WALLINT_STRIDE) = the derivative of the output of
 * adflow_gpu_wall_integrate in the direction x (n = nState x owned cells of the level), by ONE pass seeded with x through the
 * 2-layer exchange; out, where not NULL, takes the value parts (the integration itself, from the stress of this pass).
 *
 * adflow_gpu_wall_integrate_bwd[_dev]: outBar = nRhs weight sets of nGroups x ADFLOW_WALLINT_STRIDE doubles (what getCostFunctions_b
 * makes of funcsBar), set r at outBar + r nGroups ADFLOW_WALLINT_STRIDE, ALWAYS in host memory; wbar = nRhs vectors ld doubles apart
 * (ld >= n; the padding is not touched): column r = sum over groups g and entries e of outBar_r[g, e] d out[g, e] / d w, the right-hand
 * side of the adjoint for adflow_gpu_gmres_solve(transpose) or adflow_gpu_gmres_solve_multi.  A coloured sweep of the pass above: 125
 * colours (i mod 5, j mod 5, k mod 5 of the block-local index, halos included) x nState variables, every pass serving all weight sets;
 * per pass the derivative parts of a face's terms are contracted with the weights of its groups and gathered -- per cell, in a fixed
 * order, no atomics -- onto the one cell of the colour in the face's stencil; halo cells are then added to their donors by the
 * reverse exchange of adflow_gpu_jacobian_mult (a halo without a donor is no column).  Bit-identical from call to call.
 * The _dev forms take device pointers for x, out, outDot and wbar and honour adflow_gpu_set_async; they wait for the queue only
 * where buffers are laid out or the weights or family lists differ from those of the previous call.
 * Errors: everything adflow_gpu_wall_integrate (but for a stress never stored) and adflow_gpu_jacfree_mult refuse; ADFLOW_JAC_PC,
 * ADFLOW_JAC_VISC_PC, ADFLOW_JAC_APPROX_SA (approximations of fluxes this path does not run); n of the wrong length; a NULL vector;
 * a nonzero weight on entry 17 or 63; nRhs < 1 or > ADFLOW_GPU_MAX_NVEC; ld < n; halos exchanged with other ranks (bwd).  A level
 * without a wall subface is no error: zeros.
 * Buffers: the partial results, the halo'd result of the sweep (nState x nRhs doubles per box cell) and the contracted derivatives
 * belong to the level's integration record: released and counted by adflow_gpu_release_workspace, dropped by
 * adflow_gpu_bc_register and adflow_gpu_bc_set_families; the dual arrays are those of adflow_gpu_jacfree_mult.
 * Not here: derivatives with respect to the mesh and the flight condition (xvbar, extraBar), nodal force seeds, several ranks. */
enum {
    ADFLOW_WALLINT_MACHCOEF = 0,
    ADFLOW_WALLINT_POINTREF = 1,             /* pointRef(3) */
    ADFLOW_WALLINT_MOMENTAXIS = 4,           /* momentAxis(3,2), column-major: the first point, then the second */
    ADFLOW_WALLINT_VELDIRFREESTREAM = 10,    /* velDirFreeStream(3) */
    ADFLOW_WALLINT_SEPSENSOROFFSET = 13,
    ADFLOW_WALLINT_SEPSENSORSHARPNESS = 14,
    ADFLOW_WALLINT_COMPUTECAVITATION = 15,   /* 0 / 1 */
    ADFLOW_WALLINT_CAVITATIONNUMBER = 16,
    ADFLOW_WALLINT_CAVSENSOROFFSET = 17,
    ADFLOW_WALLINT_CAVSENSORSHARPNESS = 18,
    ADFLOW_WALLINT_CAVEXPONENT = 19,         /* a whole number >= 0 */
    ADFLOW_WALLINT_CPMIN_RHO = 20,
    ADFLOW_WALLINT_CPMIN_FAMILY = 21,
    ADFLOW_WALLINT_NPAR = 22
};
#define ADFLOW_WALLINT_STRIDE 64
#define ADFLOW_WALLINT_CPMIN 63              /* entry of a group's output that holds the minimum of Cp */
int adflow_gpu_bc_set_families(int nn, int level, int sps, int nBocos, const int32_t* famID, const int8_t* const* iblank);
int adflow_gpu_wall_integrate(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out);
int adflow_gpu_wall_integrate_dev(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out);
int adflow_gpu_download_wall_forces(int nn, int level, int sps, int mm, double* Fp, double* Fv, double* area);
int adflow_gpu_wall_integrate_fwd(int level, unsigned flags, const double* x, long n, const double* par, int nGroups,
                                  const int32_t* famLists, int ldFam, double* out, double* outDot);
int adflow_gpu_wall_integrate_fwd_dev(int level, unsigned flags, const double* d_x, long n, const double* par, int nGroups,
                                      const int32_t* famLists, int ldFam, double* d_out, double* d_outDot);
int adflow_gpu_wall_integrate_bwd(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                  const double* outBar, int nRhs, double* wbar, long n, long ld);
int adflow_gpu_wall_integrate_bwd_dev(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                      const double* outBar, int nRhs, double* d_wbar, long n, long ld);
/* ---- flow integration: mass flow and flow properties over in- and outflow faces -------------------------------------------------------
 * adflow_gpu_flow_integrate[_dev]: flowIntegrationFace (surfaceIntegrations.F90:894-1200) over the SubsonicInflow, SupersonicInflow,
 * SubsonicOutflow and SupersonicOutflow subfaces of a level, the other half of integrateSurfaces (:1303-1361).  par =
 * ADFLOW_FLOWINT_NPAR doubles at the indices below: what the routine reads and adflow_gpu_set_options does not carry (pInf, pRef,
 * gammaInf, RGas, TRef, uRef, timeRef and LRef come from there).  nGroups, famLists, ldFam, out: as for adflow_gpu_wall_integrate,
 * families and blanking from adflow_gpu_bc_set_families; nGroups = 0 = one group holding every in- and outflow subface.  Entries of a
 * group's output, at the reference's indices: iMassFlow, iMassPtot, iMassTtot, iMassPs, iMassMN, iMassa, iMassRho, iMassVx/Vy/Vz,
 * iMassnx/ny/nz, iMassVi, iArea, iAreaPTot, iAreaPs, iFp(3), iFlowMp(3), iFlowFm(3), iFlowMm(3), iCoForceX/Y/Z(3); every other slot
 * (entry 63 included) is zero.  iFp and iCoForce* are shared with the wall integration as in the reference: the host adds the two
 * vectors before its mpi_allreduce and getCostFunctions.  The terms are the reference's: fact +1 on min faces, inFlowFact -1 on the two
 * inflow kinds, blk = max(iblank, 0), means of halo and first interior cell, sF from sFace on a block with grid velocities, vmag =
 * sqrt(v . v) - sF, Ptot / Ttot of computePtot / computeTtot for constant cp, pratio = min(1, 1 / Ptot).  Reads the halos as the last
 * boundary-condition pass left them, changes neither state nor residual nor anything of the wall integration; two-pass sums in a
 * fixed order, no atomics: bit-identical from call to call and between the two forms.  The _dev form takes a device pointer for out
 * and honours adflow_gpu_set_async; it waits for the queue only when the family lists differ from those of the previous call.
 * Errors (nothing is launched or allocated): a level without registered boundary subfaces; nGroups < 0; a family count above
 * ldFam - 1; rhoRef or rGasDim not positive.  A level without an in- or outflow subface is no error: zeros.
 *
 * adflow_gpu_flow_integrate_fwd[_dev], _bwd[_dev]: the derivatives with respect to the state, arguments and layout as for
 * adflow_gpu_wall_integrate_fwd / _bwd.  The pass runs the closures and the dual flow boundary conditions and nothing else (no
 * turbulence boundary condition, no nodal gradient: the terms read rho, the velocities, p and gamma of the halo and the first interior
 * cell), then the face terms on dual numbers; _bwd is the same coloured sweep (125 colours x nState) with the same per-cell gather.
 * out of _fwd, where not NULL, is adflow_gpu_flow_integrate itself, to the bit: the plain kernels run in the same queue (the dual pass
 * forms the pressure again from the energy, its value parts agree with them to rounding only).
 * Supersonic outflow (and extrapolated) halos are not linearised by the dual boundary conditions, as in BCExtra_d.F90: on those
 * faces the halo is a constant.  ADFLOW_JAC_TURB_ONLY gives exact zeros.  Weights on entries the integration leaves zero are ignored.
 * Errors: those above and everything adflow_gpu_wall_integrate_fwd / _bwd refuse (the approximating flags, a wrong n, NULL vectors,
 * nRhs out of range, ld < n, halos exchanged with other ranks in _bwd; moving blocks, which the dual kernels do not linearise).
 * Every one of them is found by the checks of the arguments, before the level's record is looked up or built: a refused call of
 * the derivative entries has launched and allocated nothing either.
 * Buffers: a record per level beside that of the walls, with the same lifetime: allocated by the first call that needs them, freed
 * and counted by adflow_gpu_release_workspace, dropped by adflow_gpu_bc_register, adflow_gpu_bc_set_families,
 * adflow_gpu_block_release and adflow_gpu_release_all.
 * Not here: xvbar / extraBar, zippers, user surfaces, actuator regions, mass-bleed outflow, getCostFunctions, several ranks in _bwd. */
enum {
    ADFLOW_FLOWINT_POINTREF = 0,             /* pointRef(3) */
    ADFLOW_FLOWINT_INTERNALFLOW = 3,         /* 0 / 1: flowType == internalFlow (the momentum force and moment change sign) */
    ADFLOW_FLOWINT_RHOREF = 4,               /* flowVarRefState::rhoRef */
    ADFLOW_FLOWINT_RGASDIM = 5,              /* inputPhysics::rGasDim */
    ADFLOW_FLOWINT_NPAR = 6
};
int adflow_gpu_flow_integrate(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out);
int adflow_gpu_flow_integrate_dev(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out);
int adflow_gpu_flow_integrate_fwd(int level, unsigned flags, const double* x, long n, const double* par, int nGroups,
                                  const int32_t* famLists, int ldFam, double* out, double* outDot);
int adflow_gpu_flow_integrate_fwd_dev(int level, unsigned flags, const double* d_x, long n, const double* par, int nGroups,
                                      const int32_t* famLists, int ldFam, double* d_out, double* d_outDot);
int adflow_gpu_flow_integrate_bwd(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                  const double* outBar, int nRhs, double* wbar, long n, long ld);
int adflow_gpu_flow_integrate_bwd_dev(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                      const double* outBar, int nRhs, double* d_wbar, long n, long ld);
/* Actuator regions (actuatorRegionData.F90): residuals::sourceTerms_block (residuals.F90:348-425) adds the body force and
 * heat source of every listed cell to dw of the FINE level: -vol * force / volume / pRef on the momentum residuals,
 * -(F . v) - vol * heat / volume / (pRef uRef LRef^2) on the energy residual, ramped by ordersConverged between
 * relaxStart and relaxEnd.  Once regions are registered every level-1 residual evaluation of the library includes
 * them where the reference calls sourceTerms (smoothers.F90:74,409, multiGrid.F90:52,887,949, blockette.F90:278);
 * the body of the host's `sourceTerms` shell becomes a no-op like `initres`.  block(:) = local block nn of each cell
 * (what blkPtr encodes), cellIDs (3,nCellIDs) column-major.  nRegions = 0 removes them. */
typedef struct adflow_actuator_region {
    int32_t nCellIDs, reserved;
    const int32_t *block, *cellIDs;
    double force[3], heat, volume, relaxStart, relaxEnd;
} adflow_actuator_region;
int adflow_gpu_actuator_register(int nRegions, const adflow_actuator_region* regions);
/* sum over owned cells of (dw(:,l)/vol)^2, l=1..n  (solvers.F90:1538) */
int adflow_gpu_res_norms(int level, double* sums, int n);

/* ---- Newton-Krylov glue (src/NKSolver/NKSolvers.F90) -----------------------
 * vectors are the PETSc layout: block, k, j, i, variable fastest; n = total DOF of
 * the level-1 blocks of this process (nw * owned cells).  Host-pointer forms copy
 * through PCIe; *_dev forms take device pointers (PETSc VECHIP). */
int adflow_gpu_set_w_vec(const double* wVec, long n);                 /* setW :1331 (turbulence clipped at 1e-6*wInf) */
int adflow_gpu_get_r_vec(double* rVec, long n, double* sumsq2);        /* setRVec :1262: dw/volRef, turb*turbResScale; sumsq2[0..1] = sum flow^2, turb^2 (may be NULL) */
int adflow_gpu_get_res(double* res, long n);                           /* nksolver::getRes :1413: no turbResScale */
/* FormFunction_mf (:437-461): setW + blocketteRes(all defaults) + setRVec */
int adflow_gpu_nk_residual(const double* wVec, double* rVec, long n);
int adflow_gpu_nk_residual_dev(const double* d_wVec, double* d_rVec, long n);

/* ---- instrumentation: HIP events on the library's own stream ------------ */
int adflow_gpu_event_record(int slot);                   /* slot in [0,64) */
int adflow_gpu_event_elapsed_ms(int slot_start, int slot_stop, double* ms);
int adflow_gpu_sync(void);
/* wavefront-steps (wavefronts x k-planes marched) one evaluation of `level` costs each marching kernel, for the FP64-issue roofline of
 * bench.py (steps x the instruction count of the kernel's main loop, profiles/isa_counts.json): out[0] Spalart-Allmaras march,
 * [1] fused nodal gradients + viscous fluxes, [2] inviscid / viscous marches over the tile table, [3] reserved (0);
 * n >= 4.  Geometry only, no device work. */
int adflow_gpu_march_stats(int level, double* out, int n);
/* performance knobs for A/B measurements; results never depend on them.
 * "euler_march" (default 1): k-marching fused kernel for Euler + scalar JST; the full list with defaults: DESIGN.md section 8b */
int adflow_gpu_set_tuning(const char* key, int value);
/* on != 0: hot-path entry points only ENQUEUE on the library stream (no host
 * sync at return); the caller orders with adflow_gpu_sync().  Default off.
 * The mode covers device work only.  An entry that takes a pointer to a HOST array of the caller (the upload_ / download_ entries,
 * the host forms of the vector entries, bc_register, comm_register, wall_distance_register, update_wall_distances, halo_pack /
 * halo_unpack, mg_cycle's cycling) has consumed -- or filled -- that array when it returns, in either mode and also when it returns
 * an error: the caller may reuse or free it at once.  Only the _dev forms, whose vectors live on the device, leave reads and writes
 * of their arguments in the queue; those are ordered by the stream, and by adflow_gpu_sync() against the host.  An entry that hands
 * a value back to the host (a norm, lambda, an iteration count, ank_last_h) synchronises whatever the mode is. */
int adflow_gpu_set_async(int on);
/* sizeof(adflow_opts), sizeof(adflow_block_desc) as compiled: lets a foreign-
 * language binding verify its mirror of the two structs */
int adflow_gpu_abi_sizes(int* opts_bytes, int* desc_bytes);
/* the same for adflow_bc_subface and adflow_comm_pattern */
int adflow_gpu_abi_sizes2(int* bc_subface_bytes, int* comm_pattern_bytes);

/* ---- preconditioner / Jacobian assembly: adjointUtils::setupStateResidualMatrix with useAD = F (src/adjoint/adjointUtils.F90:7-715),
 * consumers NKSolver::FormJacobianNK (NKSolvers.F90:372-435), FormJacobianANK (:1935-2039), the adjoint's dRdwT.
 * Coloured finite differences of the level's residual (block_res_state, masterRoutines.F90:1214-1283: closures incl. halos,
 * boundary conditions, residual core, resScale) on the device: one residual evaluation per colour and state variable fills one
 * column of every stencil block of the matrix.
 *   ADFLOW_JAC_PC          usePC: 7-point stencil, lumped dissipation with the frozen sensor, thin-layer viscous flux,
 *                          first-order turbulence advection, acousticScaleFactor = 1 (7 colours)
 *   without it             the exact dR/dw: 13-point stencil / 13 colours (Euler), 33-point stencil / 35 colours (viscous)
 *   ADFLOW_JAC_FROZEN_TURB frozenTurb: nState = nwf, RANS evaluated as laminar NS plus the eddy viscosity, no SA residual
 *   ADFLOW_JAC_TURB_ONLY   useTurbOnly (the turbulence KSP of ANK, NKSolvers.F90:2340-2370): nState = 1, only the SA residual
 *   ADFLOW_JAC_VISC_PC     inputAdjoint::viscPC with ADFLOW_JAC_PC: the 27-point stencil and the 3x3x3 colouring
 * delta: the finite-difference step (the reference uses 1e-9).  The state is restored afterwards, dw holds the scaled reference
 * residual (resetFDReference).  level must be the ground level.
 *   ADFLOW_JAC_USE_AD      useAD = T (adjointUtils.F90:227-409): every column from ONE forward-mode evaluation (seed 1 on the state
 *                          variable of the colour's cells, masterRoutines::block_res_state_d) instead of a finite difference: the
 *                          exact derivative, `delta` is not used.  Dual-number twins of the gather kernels (csrc/kernels_ad.hip).
 *                          The dual copies of the level's arrays (about 640 B per box cell) are one slab that is KEPT between calls
 *                          and freed with the blocks (adflow_gpu_block_release / _release_all) or by tuning "ad_cache" = 0; the call
 *                          fails with a message when the device has not that much memory free.
 *   ADFLOW_JAC_APPROX_SA   the SA residual of the coloured evaluations, finite-difference and forward-mode, runs with
 *                          ADFLOW_RES_APPROX_SA: the matrices FormJacobianANK (:1978) and FormJacobianANKTurb (:2364) assemble
 *                          while approxSA is set.  No effect without an SA residual (Euler / NS, ADFLOW_JAC_FROZEN_TURB).
 */
enum { ADFLOW_JAC_PC = 1u, ADFLOW_JAC_FROZEN_TURB = 2u, ADFLOW_JAC_TURB_ONLY = 4u, ADFLOW_JAC_VISC_PC = 8u, ADFLOW_JAC_USE_AD = 16u,
       ADFLOW_JAC_APPROX_SA = 32u };
int adflow_gpu_fd_jacobian(int level, unsigned flags, double delta);
/* Hands back the work space an assembly keeps between calls -- the slab of dual arrays of ADFLOW_JAC_USE_AD (about 640 B per box cell:
 * 8.4 GB on the 8 x 160x128x64 mesh) -- and the scratch arrays of adflow_gpu_jacobian_mult and adflow_gpu_jacfree_mult to the device allocator: what the host calls when the matrix is assembled and the memory is
 * wanted elsewhere (PETSc objects, further multigrid levels).  *bytes (may be NULL): what was released.  The next forward-mode
 * assembly lays the slab out again.  Mirrors nothing in the reference, whose Tapenade derivative arrays live in flowDomsd for the
 * whole run (adjointUtils.F90:87-99 allocDerivativeValues).  The buffers of adflow_gpu_wall_integrate are freed and counted too. */
int adflow_gpu_release_workspace(int64_t* bytes);
/* Self-test of the arithmetic the kernels substitute for the compiler's division, square root, pow and exp (csrc/internal.h: v_rcp_f64 /
 * v_rsq_f64 seeds + Newton steps, x^(1/6), x^a, exp of a negative argument) and of their dual-number forms (csrc/kernels_ad.hip): for
 * every i < n   y[i] = f(x[i])  by the plain form and  dy[2i], dy[2i+1] = value and d/dx by the dual form.  which: 0 1/x, 1 1/sqrt(x),
 * 2 sqrt(x), 3 x^(1/6), 4 exp(x) for x <= 0, 5 x^a[i], 6 a[i]/x, 7 x/a[i].  Host pointers.  Mirrors nothing in the reference (its
 * compiler's own division and intrinsics, e.g. sa.F90:245-330, solverUtils.F90:292-310): the check that the substitution stays inside
 * the parity bar on the arguments the flow kernels see, which the CPU emulator of the tests cannot make (it runs libm). */
int adflow_gpu_selftest_math(int which, const double* x, const double* a, int64_t n, double* y, double* dy);
/* nState, nStencil and the stencil offsets (nStencil,3) column-major as src/modules/stencils.f90 of the last assembly:
 * block (ll, l) of stencil entry s at row cell (i,j,k) is  d dw(i,j,k,ll) / d w(i-di(s), j-dj(s), k-dk(s), l)  (after resScale) */
int adflow_gpu_jacobian_info(int32_t* nState, int32_t* nStencil, int32_t* stencil);
/* blocks of block nn over its OWNED cells: (nx, ny, nz, nState, nState, nStencil) column-major.  The host maps rows / columns to
 * globalCell and calls MatSetValuesBlocked; entries whose source cell lies outside 0..ib are zero */
int adflow_gpu_download_jacobian(int nn, int level, int sps, double* blocks);
/* the same blocks in the order of the reference's insertion loop (adjointUtils.F90:560-700, one MatSetValuesBlocked per row cell
 * and stencil entry with MAT_ROW_ORIENTED off): rows(nState, nState, nStencil, nx, ny, nz) column-major, i.e. the nStencil
 * blocks blk(ll, l) of a row cell are contiguous and the cells follow in the order of the PETSc rows of the block (i fastest).
 * Transposed on the device, copied in slabs of k planes */
int adflow_gpu_download_jacobian_rows(int nn, int level, int sps, double* rows);
/* y = J x (transpose = 0) or y = J^T x (transpose != 0) with the matrix of the last successful adflow_gpu_fd_jacobian, across the
 * blocks of `level` (the level of the assembly): MatMult on dRdw / dRdwT, the operation solveAdjoint's GMRES is made of
 * (adjointAPI.F90:661-863, MatMult :741 / :806; dRdwTMatMult :1007, dRdwMatMult :1050) -- the blocks never leave the device.
 * Vectors: the layout of adflow_gpu_set_w_vec / _get_r_vec (block, k, j, i, variable fastest) with nState (not nw) variables per
 * owned cell, n = nState x owned cells of the level; host pointers, or device pointers for the _dev form (PETSc VECHIP).
 *   transpose = 0: y(row) = sum_s B_s(row) x(row - d_s)          transpose != 0: y(col) = sum_s B_s(col + d_s)^T x(col + d_s)
 * with B_s(row) the block of stencil entry s as adflow_gpu_jacobian_info documents it.  A column on a halo cell is the owned cell
 * that halo has as donor in the 2-layer cell pattern of adflow_gpu_comm_register(level, 2, ...) (same process or another rank);
 * a halo without a donor is no column (the insertion loop of the reference, adjointUtils.F90:560-700: globalCell >= 0).  The
 * transposed product adds every halo's contribution to its donor through a donor-sorted list: the result does not depend on
 * the execution order.  Periodic translations need nothing; a registered ROTATIONAL periodicity is an error when the matrix
 * covers the mean-flow variables.  State, residual and matrix are not touched; x and y must differ.  Scratch arrays of
 * 2 x nState doubles per box cell are kept between calls and released by adflow_gpu_release_workspace (which counts them in
 * *bytes) and with the blocks.  Honours adflow_gpu_set_async (the _dev form). */
int adflow_gpu_jacobian_mult(int level, int transpose, const double* x, double* y, long n);
int adflow_gpu_jacobian_mult_dev(int level, int transpose, const double* d_x, double* d_y, long n);
/* Block ILU(0) of the assembled 7-point preconditioner matrix, factored and applied on the device: the PCApply of the KSP that
 * setupStandardKSP builds (adjointUtils.F90:1374-1562) in the configuration PCBJACOBI (PCASM with overlap 0), one subdomain per
 * structured block, sub-preconditioner ILU with 0 levels of fill and the natural ordering (k, j, i with i fastest: the rows of
 * adflow_gpu_set_w_vec) on BAIJ blocks of size nState.  A column on a halo cell, with or without a donor, is not part of a
 * subdomain: the preconditioner is local to the rank whatever the number of ranks.
 *   D_c = A_cc - sum_lower A_{c,n} D_n^-1 A_{n,c},   L_{c,n} = A_{c,n} D_n^-1,   U_{c,n} = A_{c,n},   M = L (D + U)
 * over the neighbours n = c - e_i, c - e_j, c - e_k inside the block; M^T has the pivot blocks D_c^T, so one setup serves
 * z = M^-1 r (transpose = 0) and z = M^-T r (transpose != 0).  Setup and both triangular sweeps run hyperplane i + j + k by
 * hyperplane, one launch per hyperplane over every block of the level (2 x nPlanes launches per application).
 * adflow_gpu_pc_setup factors the matrix of the last adflow_gpu_fd_jacobian on `level`; it is an error unless that matrix has the
 * 7-point stencil (ADFLOW_JAC_PC without ADFLOW_JAC_VISC_PC), or when a pivot block is singular or not finite (the message names
 * block and cell; no factor is kept).  The factor owns its data -- six off-diagonal blocks and D^-1 per owned cell, 7 nState^2 x
 * 8 B, in hyperplane order, plus index tables of 36 B per cell and one vector -- and survives later assemblies: the adjoint
 * assembles the preconditioner matrix, calls adflow_gpu_pc_setup, then assembles the exact matrix.  It is released by
 * adflow_gpu_pc_release (*bytes, may be NULL: what was released, 0 without a factor), adflow_gpu_block_release and
 * adflow_gpu_release_all; adflow_gpu_release_workspace does not touch it.  adflow_gpu_pc_info: nState and the number of
 * hyperplanes of the factor and the bytes it holds; an error without a factor.
 * Vectors as for adflow_gpu_jacobian_mult (n = nState x owned cells of the level); host pointers, or device pointers for the _dev
 * form, which honours adflow_gpu_set_async.  r and z must differ.  State, residual and matrix are not touched.
 * Levels of fill (PCFactorSetLevels of setupStandardKSP, adjointUtils.F90:1559; the reference's ANKPCILUFill, NKPCILUFill and
 * ILUFill default to 2): adflow_gpu_pc_set_fill(fill) sets the fill that the next adflow_gpu_pc_setup / _ank_pc_setup of the
 * SELECTED slot uses: 0 (the default), 1 or 2; anything else is an error.  A factor that exists keeps the fill it was built with.
 * In the natural ordering the ILU(1) / ILU(2) pattern of a structured block is a fixed stencil of 13 / 23 offsets cut at the faces
 * of the block (from fill 3 on it is not, hence the limit); the factor then holds 13 / 23 blocks of nState^2 per cell and a
 * neighbour table of 12 / 22 columns, and setup and sweeps run over the level sets of the row dependencies (nx + 2 ny + 3 nz - 5
 * of them for a block at fill 1, nx + 3 ny + 7 nz - 10 at fill 2) in place of the hyperplanes.  Everything that takes a factor
 * takes one of any fill.  adflow_gpu_pc_info reports the number of level sets as nPlanes and the true bytes;
 * adflow_gpu_pc_info2: the fill of the selected factor, its entries per row (7, 13 or 23) and its number of level sets (each may
 * be NULL); an error without a factor.  An allocation that fails leaves no factor, and the message names the size.
 * Out of scope for these block-local factors: fill > 2 and the RCM ordering (the reference's default ordering; the ILU over the
 * whole level takes it: adflow_gpu_pc_set_ordering below), ASM overlap and couplings across blocks.  (The
 * pseudo-time diagonal term of ANK: adflow_gpu_ank_pc_setup below, into the same factor slot.) */
int adflow_gpu_pc_setup(int level);
int adflow_gpu_pc_info(int32_t* nState, int32_t* nPlanes, int64_t* bytes);
int adflow_gpu_pc_set_fill(int fill);
int adflow_gpu_pc_info2(int32_t* fill, int32_t* nEntries, int32_t* nLevelSets);
/* The subdomain of the ILU(0).  adflow_gpu_pc_set_coupled(coupled) sets what the next adflow_gpu_pc_setup / _ank_pc_setup of the SELECTED
 * slot builds; it is kept per slot across setups and releases, default 0; a factor that exists keeps what it was built with.
 *   0  one subdomain per structured block (PCBJACOBI): every column behind a block face is dropped from M.
 *   1  one subdomain for the level, the ASM subdomain setupStandardKSP gives a process (adjointUtils.F90:1374-1562): the 7-point matrix
 *      of the whole level is factored.  A column on a first-layer face halo whose donor in the registered 2-layer pattern of the level
 *      is an owned cell of this process is the column of that donor cell, as adflow_gpu_jacobian_mult reads it -- interfaces to another
 *      block, to the block itself (translational periodicity), rotated interfaces.  A halo without such a donor (boundary faces, halos
 *      fed by messages from other ranks) stays outside M.  Ordering: the PETSc layout, block after block in ascending nn, then k, j, i.
 *      Fill 0.  Everything that takes a factor takes this one (pc_apply[_dev], the _multi entries with up to four columns per chain of
 *      launches, gmres_solve, ank_solve, both slots, the enqueue-only mode); adflow_gpu_pc_info counts its one extra table (a word
 *      per cell, nPlanes = the level sets of the whole level), adflow_gpu_pc_release frees it.
 * Errors of the setup with coupled = 1, each with a message; the selected slot then keeps no factor, the other slot is untouched:
 * a fill > 0 set for the slot; adflow_gpu_pc_set_mg levels > 1 set for the slot; a cell that has the same column behind two faces
 * (a block periodic onto itself over fewer than three cells); a cell that has itself as a column; two neighbours of one cell that
 * are neighbours of each other (an edge with three blocks around it); a column that does not have the cell as a column in return;
 * a rotational periodicity on the pattern when the matrix covers the velocities (as adflow_gpu_jacobian_mult).
 * adflow_gpu_pc_set_coupled refuses any value but 0 and 1.
 * adflow_gpu_pc_coupled_info: of the selected factor, whether it spans the level, its level sets and the number of entries of M whose
 * column lies behind a block face (0 for a block-local factor); each may be NULL; an error without a factor. */
int adflow_gpu_pc_set_coupled(int coupled);
int adflow_gpu_pc_coupled_info(int32_t* coupled, int32_t* nLevelSets, int64_t* nCrossEntries);
/* ILU(k) over the whole level.  adflow_gpu_pc_set_level_fill(fill), fill = -1 (default: off), 0, 1, 2 or 3: with fill >= 0 the next
 * adflow_gpu_pc_setup / _ank_pc_setup of the SELECTED slot builds the ILU(fill) of the 7-point matrix of the WHOLE level -- what
 * setupStandardKSP gives one process: one ASM subdomain, PCFactorSetLevels(ILUFill / ANKPCILUFill / NKPCILUFill, default 2).  Columns
 * and ordering are those of coupled = 1 above.  The host runs the symbolic ILU(k) of the cell graph of the level once; the device
 * factors by IKJ restricted to that pattern (csrc/kernels_pc_level.hip) and sweeps over whatever rows come out (7 to 37 entries at
 * fill 2 across interfaces), so an edge with three blocks around it and a period of three cells, which coupled = 1 refuses, are
 * factored.  The storage is proportional to the entries of the pattern.  adflow_gpu_ank_pc_setup adds T as for every other factor.
 * Kept per slot across setups and releases; a factor that exists keeps what it was built with; any other value is an error that
 * names it and changes nothing.  With -1 in both slots every other path is what it was, bit for bit.
 * Everything that takes a factor takes this one: pc_apply[_dev] with and without transpose from the one factor, gmres_solve,
 * ank_solve, jacfree_solve, both slots, the enqueue-only mode, the _multi entries column by column (as at fill 2).
 * Errors of the setup, each with a message, decided before anything is allocated; the slot then keeps no factor, the other slot is
 * untouched: coupled = 1, a fill > 0 or a hierarchy set for the same slot; a matrix that is not 7-point; the same column behind two
 * faces of a cell; a cell that is its own column; a pattern entry without its mirror entry (a column that does not lead back); a
 * rotational periodicity when the matrix covers the velocities; a row of more than 65535 entries.
 * Tables once: a setup into a slot that holds such a factor of the same level, fill and nState, with no block or comm pattern
 * registered or released since, keeps the tables and redoes the numbers only (reused = 1).
 * On such a factor adflow_gpu_pc_info gives nState, the level sets and the bytes held, adflow_gpu_pc_info2 the fill, the longest row
 * and the level sets, adflow_gpu_pc_coupled_info 1, the level sets and nCrossEntries.
 * adflow_gpu_pc_level_info: the fill, the longest row, the blocks of the pattern over all rows (diagonal included), the level sets, the
 * entries of the assembled matrix whose column lies behind a block face, and reused; each may be NULL; an error without such a factor. */
int adflow_gpu_pc_set_level_fill(int fill);
int adflow_gpu_pc_level_info(int32_t* fill, int32_t* maxRow, int64_t* nEntries, int32_t* nLevelSets, int64_t* nCrossEntries, int32_t* reused);
/* The ordering of the ILU over the whole level: PCFactorSetMatOrderingType(subpc, localMatrixOrdering) of setupStandardKSP
 * (adjointUtils.F90:1555; the reference's matrixOrdering defaults to "RCM").  adflow_gpu_pc_set_ordering(kind) sets what the next
 * adflow_gpu_pc_setup / _ank_pc_setup of the SELECTED slot builds; kept per slot across setups and releases, like the fill; a factor
 * that exists keeps what it was built with; any other value is an error that names it and changes nothing.
 *   0  natural (the default): block after block in ascending nn, then k, j, i.  Tables, results and bytes are what they were.
 *   1  reverse Cuthill-McKee, computed by the library on the host: the symmetric cell graph of the 7-point pattern of the level,
 *      interface columns included, without the diagonal, the neighbours of a cell in ascending natural number; GENRCM of George and
 *      Liu: the connected components in the order of their lowest-numbered cell; per component a pseudo-peripheral root (the rooted
 *      level structure from the start cell; while it has more than one level and fewer levels than cells: the first cell of smallest
 *      degree in the last level becomes the root, and the search ends when its structure has no more levels than the one
 *      before), Cuthill-McKee from the root (cells visited in the order numbered, the unnumbered neighbours of each appended in
 *      adjacency order and that run sorted by degree, ascending and stable), reversed.  PETSc's MATORDERINGRCM calls SPARSEPACK's
 *      routine of that name; identity with the index set PETSc returns is NOT claimed.  A host that wants PETSc's numbers uses kind 2.
 *   2  the caller's permutation: adflow_gpu_pc_set_ordering_perm(perm, n), perm[new] = old, 0-based, old = the cell number of the PETSc
 *      layout of the level (a row of adflow_gpu_set_w_vec divided by nState).  The array is copied: it is consumed on return.  Errors,
 *      which name the first offending index and keep the previous permutation: n < 1, a value outside 0 .. n-1, a value that occurs
 *      twice.  perm = NULL drops the stored permutation.  Meant for the indices of the IS of PETSc's own MatGetOrdering on the local
 *      matrix: the factor then has the reference's ordering whatever PETSc's RCM does; nested dissection, minimum degree or a
 *      colouring pass the same way.
 * With P the permutation, (P A P^T)[a, b] = A[perm[a], perm[b]]: the setup builds M = ILU(fill) of P A P^T (P (A + T) P^T for
 * adflow_gpu_ank_pc_setup) and the application is z = P^T M^-1 P r, z = P^T M^-T P r for the transpose; the caller's vectors stay in
 * the PETSc layout.  The symbolic ILU(k), the ascending columns of a row, the pivot order, the level sets and the storage order run
 * in the ordered numbering; the columns and the setup refusals of the factor over the level are unchanged.  Everything that takes a
 * factor takes an ordered one, adflow_gpu_pc_set_its included (its products on A_full stay in the natural layout).
 * Errors of the setup, each with a message; the slot then holds no factor, the other slot is untouched: kind != 0 while the level
 * fill of the slot is -1 (the block-local factors, coupled = 1 and the hierarchy have the fixed stencils of the natural ordering);
 * kind 2 without a stored permutation; kind 2 with n different from the owned cells of the level.
 * Tables once: reused = 1 also needs the same kind and, for kind 2, no adflow_gpu_pc_set_ordering_perm since the tables were
 * built.  The RCM ordering is recomputed only when the tables are.
 * adflow_gpu_pc_ordering_info, of the selected slot's factor: the kind, bandwidth = max |ordered(column) - ordered(row)| over the
 * assembled 7-point entries (interface columns included), the level sets and the blocks of the pattern; a factor that is no ILU over
 * the level reports kind 0, bandwidth -1 and its entries per row x cells; each may be NULL; an error without a factor.
 * adflow_gpu_pc_download_ordering: perm[new] = old the selected factor was built with, n = its cells (the identity for kind 0); an
 * error without a factor or with another n. */
int adflow_gpu_pc_set_ordering(int kind);
int adflow_gpu_pc_set_ordering_perm(const int32_t* perm, long n);
int adflow_gpu_pc_ordering_info(int32_t* kind, int64_t* bandwidth, int32_t* nLevelSets, int64_t* nEntries);
int adflow_gpu_pc_download_ordering(int32_t* perm, long n);
int adflow_gpu_pc_apply(int level, int transpose, const double* r, double* z, long n);
int adflow_gpu_pc_apply_dev(int level, int transpose, const double* d_r, double* d_z, long n);
int adflow_gpu_pc_release(int64_t* bytes);
/* Two factor slots (ANK_jacobianLag keeps the flow factor and the turbulence factor alive over the same steps): slot 0 or 1, default
 * 0.  adflow_gpu_pc_setup, _ank_pc_setup, _pc_set_fill, _pc_apply, _pc_info, _pc_info2, _pc_release, _gmres_solve and _ank_solve act on the
 * selected slot (each slot keeps its own fill);
 * adflow_gpu_block_release and _release_all release both.  A process that never calls it behaves as with one slot. */
int adflow_gpu_pc_select(int slot);
/* Multigrid preconditioner: the `mg` preconditioner of the reference (precondType = 'mg', amg.F90; ANKAMGLevels, NKAMGLevels,
 * adjointAMGLevels default 2, ...AMGNSmooth default 1), block-local like the factor.  A = the matrix the factor is built from: the
 * assembled 7-point matrix restricted to the columns inside the row's own block, with the pseudo-time term T on the diagonal blocks
 * when the setup is adflow_gpu_ank_pc_setup.  Levels l = 1 .. L, level 1 the fine one:
 *   sizes       per block and direction n -> n/2 if even, (n+1)/2 if odd, 1 stays 1 (amg.F90:140-155)
 *   aggregates  the fine cell (i, j, k), 0-based, of a block belongs to the coarse cell (i/2, j/2, k/2) of the same block (:222-226);
 *               the blocks follow each other in the vectors of every level in the order of level 1, natural ordering inside a block
 *   matrices    A_{l+1} = P^T A_l P, P the piecewise-constant prolongation: the plain sum of the reference's MatSetValuesBlocked(...,
 *               ADD_VALUES) on the coarse indices (adjointUtils.F90:683-710).  7-point again: the diagonal block of a coarse cell is
 *               the sum of its children's diagonal blocks and of every entry between two of them, the entry towards a neighbouring
 *               aggregate the sum of the children's entries across that face -- summed in one fixed order
 *   smoother    S_l(b) (setupShellPC: Richardson from zero, nSmooth iterations, one local ILU application each):  x = M_l^-1 b, then
 *               nSmooth - 1 times x += M_l^-1 (b - A_l x);  M_l = the block ILU of A_l in the natural ordering, with the fill of the
 *               slot (adflow_gpu_pc_set_fill) on level 1 and fillCoarse on the levels below
 *   cycle       MG(r, k) (amg.F90:712-759):  rhs = P^T r;  sol = S_{k+1}(rhs) if k + 1 = L, else MG(rhs, k + 1);  y = P sol;
 *               res = r - A_k y;  y += S_k(res).  The preconditioner is z = MG(r, 1): the coarse level first, smoothing afterwards.
 *   transpose   the same cycle on A^T, with A_l^T and M_l^-T everywhere (the reference assembles the transposed matrices into the same
 *               hierarchy); it is NOT the transpose of the cycle.
 * outerPreConIts and innerPreConIts[Coarse]: adflow_gpu_pc_set_its below.  Out of scope: couplings across blocks inside the hierarchy
 * (the outer iterations see them), ranks, ASM overlap, the RCM ordering.
 * adflow_gpu_pc_set_mg(levels, nSmooth, fillCoarse) sets what the next adflow_gpu_pc_setup / _ank_pc_setup of the SELECTED slot
 * builds; each slot keeps its own setting, like its fill.  levels = 1 (the default) is the plain factor, with nSmooth and fillCoarse
 * ignored.  Errors: levels outside 1 .. 10, nSmooth < 1, fillCoarse outside 0 .. 2.  With levels > 1 the setup builds the hierarchy
 * into the slot; it is an error, naming the level, when level l + 1 would have as many cells as level l (every block is 1 x 1 x 1
 * there); a singular pivot block names the multigrid level as well as block and cell; an allocation that fails names its size; nothing
 * is kept on failure.  The slot owns all the cycle needs: a copy of the fine in-block blocks (T included; the assembled blocks are
 * overwritten by the next assembly), the coarse matrices, one factor per level and four vectors per level.  adflow_gpu_pc_info counts
 * all of it (nPlanes: the level sets of the level-1 factor), adflow_gpu_pc_release, _block_release and _release_all free it,
 * adflow_gpu_release_workspace does not touch it.  Everything that takes a factor takes a hierarchy: adflow_gpu_pc_apply[_dev],
 * _gmres_solve[_dev], _ank_solve[_dev]; an application launches on the library's stream only, allocates nothing and does not
 * synchronise (the _dev form stays enqueue-only under adflow_gpu_set_async(1)).  The _multi entries serve the columns of a hierarchy
 * ONE AT A TIME through the single cycle, as they do at fill 2: they cost what the single calls cost.
 * adflow_gpu_pc_mg_info: levels, nSmooth, fillCoarse of the selected slot's factor (1, 1, 0 for a plain factor) and the cells of every
 * level (cells: `levels` entries; each pointer may be NULL); an error without a factor.
 * adflow_gpu_pc_mg_download: the blocks of block nn on multigrid level mgLevel, blocks(nx_l, ny_l, nz_l, nState, nState, 7)
 * column-major with the stencil order of adflow_gpu_jacobian_info -- the layout of adflow_gpu_download_jacobian; mgLevel = 1 is the
 * owned fine copy (entries whose column lies outside the block are zero).  An error without a hierarchy. */
int adflow_gpu_pc_set_mg(int levels, int nSmooth, int fillCoarse);
int adflow_gpu_pc_mg_info(int32_t* levels, int32_t* nSmooth, int32_t* fillCoarse, int64_t* cells);
int adflow_gpu_pc_mg_download(int mgLevel, int nn, double* blocks);
/* Preconditioner Richardson iterations: the two loops setupStandardKSP (adjointUtils.F90:1374-1562) wraps around the ILU, and the mg
 * shell with them (amg.F90:487-510, :534-615).  With M the factor of the selected slot and
 *   S(b; M, A, n):  x = M^-1 b, then n - 1 times x += M^-1 (b - A x)      (PETSc's Richardson from a zero guess, scale 1, no norm:
 *                                                                          n applications, n - 1 products)
 *   A_full  the 7-point matrix of the whole level as it stood at the setup (adflow_gpu_ank_pc_setup: T on the diagonal blocks): an owned
 *           cell is its own column, a first-layer face halo the owned cell it has as donor in the registered 2-layer pattern, a halo
 *           without such a donor is no column -- the matrix adflow_gpu_jacobian_mult applies for that assembly on one rank
 *   A_sub   the matrix the factor was built from: A_full without the columns behind block faces for a block-local factor (fill 0, 1, 2
 *           with coupled = 0), A_full for coupled = 1 and for adflow_gpu_pc_set_level_fill >= 0
 * a plain factor applies   local(b) = S(b; M, A_sub, inner);   P(b): y = local(b), then outer - 1 times y += local(b - A_full y)
 * (localPreConIts on the subksp of every subdomain, globalPreConIts on master_PC_KSP).  A hierarchy (levels > 1) replaces the one ILU
 * application of every smoothing iteration on level l by L_l(r) = S(r; M_l, A_l, inner_l), inner_1 = inner and inner_l = innerCoarse
 * below level 1 (amgLocalPreConIts), leaves the cycle as it is and applies P(b): y = MG(b), then outer - 1 times y += MG(b - A_full y)
 * -- the reference's fineMat is the whole matrix, so the outer product includes the columns behind block faces although the hierarchy
 * is block-local.  transpose: the same recurrences with A^T and M^-T throughout; for a plain factor that is exactly P^T, for a
 * hierarchy it is not, as before.  outer = inner = innerCoarse = 1 (the default) is every path as it was, bit for bit, holding the
 * bytes it held.
 * adflow_gpu_pc_set_its(outer, inner, innerCoarse) sets what the next adflow_gpu_pc_setup / _ank_pc_setup of the SELECTED slot builds;
 * each slot keeps its own setting across setups and releases, and a factor that exists keeps what it was built with.  A value below 1
 * is an error that names it and changes nothing.  innerCoarse is ignored with levels = 1.
 * With outer > 1, or inner > 1 on a plain factor, the setup copies the assembled 7-point blocks (T included) into storage the slot
 * owns -- the adjoint assembles the preconditioner matrix, factors it and overwrites it with the exact matrix -- with the column
 * table of the level and, for the transposed product, the mirror entries, and allocates the work vectors of the recurrences; nothing
 * is allocated at application time.  A hierarchy owns its A_l already: inner iterations on it need two vectors per level, no matrix.
 * Errors of the setup, decided before anything is allocated, with no factor kept and the other slot untouched: the same column
 * behind two faces of a cell, a cell that is its own column, a column that does not lead back; a rotational periodicity when the
 * matrix covers the velocities; an allocation that fails names its size.  adflow_gpu_pc_info counts the new bytes,
 * adflow_gpu_pc_release, _block_release and _release_all free them, adflow_gpu_release_workspace does not touch them; a setup that
 * keeps the tables of an ILU over the level (reused = 1) redoes the copy.  Every entry that takes a factor takes the iterations:
 * adflow_gpu_pc_apply[_dev], _gmres_solve[_dev], _ank_solve[_dev], _jacfree_solve[_dev], both slots, enqueue-only under
 * adflow_gpu_set_async(1); the _multi entries in groups of up to four columns where the sweeps of the factor take them, column by
 * column where they do not.
 * adflow_gpu_pc_its_info: the counts of the selected slot's factor and matrixBytes, what the owned copy of A_full and its tables
 * hold (0 when none is held); each pointer may be NULL; an error without a factor.
 * Out of scope: ASM overlap, more than one rank in the solver, KSP types other than GMRES and left
 * preconditioning, inner iterations whose subdomains differ from the factor's own. */
int adflow_gpu_pc_set_its(int outer, int inner, int innerCoarse);
int adflow_gpu_pc_its_info(int32_t* outer, int32_t* inner, int32_t* innerCoarse, int64_t* matrixBytes);
/* Restarted GMRES with the factor as RIGHT preconditioner, the KSPSolve of solveAdjoint (adjointAPI.F90:661-863) with the settings
 * of setupStandardKSP (adjointUtils.F90:1374-1562: KSPGMRES, PC_RIGHT, modified Gram-Schmidt):  A M^-1 u = b, x = M^-1 u, with
 * A = adflow_gpu_jacobian_mult on the matrix assembled last (7-, 13-, 27- or 33-point) and M = the factor of adflow_gpu_pc_setup,
 * both transposed when transpose != 0 (the adjoint: assemble the preconditioner matrix, adflow_gpu_pc_setup, assemble the exact
 * matrix, solve with transpose = 1).  Basis vectors, dot products and updates stay on the device; the Hessenberg matrix and the
 * Givens rotations are kept on the host, one download of a column per iteration.  The iteration stops when the residual of the
 * recurrence is <= max(rtol ||b||, atol), or after maxIts iterations (not an error); restart = size of the Krylov space.
 * useGuess != 0: x holds the initial guess (else it is ignored and the solve starts from 0).  *its: iterations done; *rnorm0: the
 * initial residual norm; *rnorm: the TRUE residual ||b - A x|| of the returned x, computed once at the end (each may be NULL).
 * Errors: no matrix or no factor, nState of factor and matrix differ, wrong level or n, b == x, and more than one rank in the
 * communicator of adflow_gpu_comm_init -- the dot products are not reduced across ranks (out of scope): such a host keeps its KSP
 * and calls the two _dev operators.  (The same solver on a matrix-free operator: adflow_gpu_ank_solve below.)  Work space of
 * restart + 4 vectors is allocated for the call.  State, residual, matrix and factor are not touched. */
int adflow_gpu_gmres_solve(int level, int transpose, const double* b, double* x, long n, int restart, int maxIts, double rtol,
                           double atol, int useGuess, int* its, double* rnorm0, double* rnorm);
int adflow_gpu_gmres_solve_dev(int level, int transpose, const double* d_b, double* d_x, long n, int restart, int maxIts, double rtol,
                               double atol, int useGuess, int* its, double* rnorm0, double* rnorm);
/* Matrix-free exact products by forward mode: y = (dR/dw) x without an assembled matrix.  The reference does not assemble the exact
 * matrix by default either: useMatrixFreedRdw defaults to True (pyADflow.py:5918), createPETScVars makes dRdwT a shell matrix
 * (adjointAPI.F90:1199-1214) and its forward product is dRdwMatMult (:1050-1128), ONE call of master_d with the vector as seed --
 * what solveDirectForRHS iterates on and computeJacobianVectorProductFwd(wDot = ...) returns.
 * flags: ADFLOW_JAC_PC, _FROZEN_TURB, _TURB_ONLY, _VISC_PC, _APPROX_SA with their meaning for adflow_gpu_fd_jacobian; ADFLOW_JAC_USE_AD
 * is implied and ignored.  y is the product adflow_gpu_jacobian_mult(level, 0, x, y, n) returns after adflow_gpu_fd_jacobian(level,
 * flags | ADFLOW_JAC_USE_AD, .), to rounding, linearised about the state that is on the device at the call; no assembled matrix is
 * read or written.  Vectors as for adflow_gpu_jacobian_mult, with the nState and first variable the flags select (6, 5 or 1).  Columns
 * as there: an owned cell is its own column, a halo with a donor in the 2-layer pattern of adflow_gpu_comm_register(level, 2, ...)
 * carries its donor's entry of x (same process or another rank), every other halo carries a zero seed.
 * The evaluation is the one a coloured pass of the forward-mode assembly runs: whalo2 of the state once, the frozen shock sensor
 * first under ADFLOW_JAC_PC, the switches of the preconditioner matrix for the evaluation only, block_res_state_d on the seeded dual
 * state, the result scaled by 1 / volRef and turbResScale on the turbulence row.  It works in the slab of dual arrays of
 * ADFLOW_JAC_USE_AD (shared with the assembly) and a scratch array of nState doubles per box cell, both kept between calls and
 * released -- and counted -- by adflow_gpu_release_workspace and with the blocks.  State, residual, assembled matrix and factors are
 * left as they were.  adflow_gpu_jacfree_mult prepares on every call (exchange, sensor, passive dual arrays), so it is always about
 * the current state.  The _dev form honours adflow_gpu_set_async: the host then waits only when the slab or the scratch has to be
 * laid out.
 * adflow_gpu_jacfree_solve: the restarted GMRES of adflow_gpu_gmres_solve with this product as operator and the factor of the SELECTED
 * slot as right preconditioner, never transposed -- the KSP of solveDirectForRHS on the shell dRdwT.  It prepares once; its products
 * only seed, evaluate and read out.  Arguments and results as for adflow_gpu_gmres_solve.
 * Errors, each with a message before anything is launched: what adflow_gpu_fd_jacobian refuses for ADFLOW_JAC_USE_AD (moving blocks,
 * actuator regions, host boundary hooks, a level that is not the ground level, TURB_ONLY without RANS or with FROZEN_TURB), unknown
 * flags, x == y, a wrong n, a registered ROTATIONAL periodicity when the mean-flow variables are covered; for the solve also no factor
 * in the selected slot, a factor of another nState, more than one rank, bad caps.
 * Out of scope: the transposed product (it needs reverse mode; the adjoint keeps the assembled J^T and adflow_gpu_jacobian_mult),
 * several vectors per pass, and the spatial and extra seeds of master_d (xDot, forces, functions). */
int adflow_gpu_jacfree_mult(int level, unsigned flags, const double* x, double* y, long n);
int adflow_gpu_jacfree_mult_dev(int level, unsigned flags, const double* d_x, double* d_y, long n);
int adflow_gpu_jacfree_solve(int level, unsigned flags, const double* b, double* x, long n, int restart, int maxIts, double rtol,
                             double atol, int useGuess, int* its, double* rnorm0, double* rnorm);
int adflow_gpu_jacfree_solve_dev(int level, unsigned flags, const double* d_b, double* d_x, long n, int restart, int maxIts, double rtol,
                                 double atol, int useGuess, int* its, double* rnorm0, double* rnorm);

/* ---- several right-hand sides at once: the product, the ILU application and GMRES on nvec columns -------------------------------
 * The adjoints of several functions (the loop in front of solveAdjoint, pyADflow.py:1723-1743) and the seeds of solveAdjointForRHS /
 * solveDirectForRHS (adjointAPI.F90:265-428) share one matrix and one factor; these entries take their vectors together.  Column c is
 * the n doubles at X + c ld, ld >= n, each in the layout of adflow_gpu_set_w_vec exactly like a vector of the single entries: the
 * vectors lie one behind the other (not interleaved), so a host hands over its existing Vec arrays.  Host pointers, or device
 * pointers for the _dev forms, which honour adflow_gpu_set_async where their single twins do (product and application; the solver
 * synchronises every iteration).
 * Every column behaves as the single entry does on that column -- same matrix, same selected factor slot of any fill (one of
 * adflow_gpu_ank_pc_setup included), same transposes; nvec = 1 runs the kernels of the single entry and is bit-identical to it.
 * Wider calls run kernels that read every matrix or factor block once for up to 4 vectors and go through the level sets once;
 * more than 4 columns are served in groups of 4 and a rest (7 = 4 + 3), at most ADFLOW_GPU_MAX_NVEC per call (a factor of fill 2
 * is applied column by column with the kernels of one vector).  Their results
 * agree with the single entries to rounding, and a column does not depend on what the other columns hold.
 *   adflow_gpu_jacobian_mult_multi   Y_c = J X_c (J^T X_c), one pass over the matrix per group.  The scratch arrays of the product
 *                          grow to the widest group used (adflow_gpu_release_workspace counts and frees them as before).
 *   adflow_gpu_pc_apply_multi        Z_c = M^-1 R_c (M^-T R_c), one launch per level set for all blocks and all columns of a group.
 *                          The work space of the other vectors of a group is allocated at the first multi application of a factor
 *                          and kept at the widest group used: it belongs to the factor, adflow_gpu_pc_info counts it from then
 *                          on, and it is released with the factor.  A process that never calls a multi entry holds the bytes it
 *                          always held.
 *   adflow_gpu_gmres_solve_multi     nvec independent right-preconditioned GMRES(restart) iterations in lock-step: one multi
 *                          application and one multi product per iteration, every launch of the Gram-Schmidt chain for all columns
 *                          (partial sums per column, added in the order of the single solver), one download and one synchronise per
 *                          iteration.  Tolerance max(rtol ||B_c||, atol), Hessenberg matrix, rotations and count are per column, and a
 *                          column stops where its own adflow_gpu_gmres_solve would (tolerance met, breakdown, maxIts): its X_c is
 *                          formed from its own Krylov space at that iteration and not touched afterwards, while the others go on.
 *                          The restart boundaries are shared (every column starts at iteration 0).  its, rnorm0, rnorm: nvec entries
 *                          each, each may be NULL; rnorm[c] is the true residual of X_c.  Work space of (restart + 3) nvec vectors
 *                          is allocated for the call; if that fails the error names the size and nothing is held.
 * Errors: everything the single entries refuse, named by the multi entry; nvec < 1 or > ADFLOW_GPU_MAX_NVEC; ld < n; a column of the
 * input that shares memory with a column of the result (column a of the one with column b of the other included); for the solver a
 * right-hand side that is not finite (the column is named) and more than one rank.
 * Out of scope: the ANK entries stay single-vector (adflow_gpu_ank_mult is one residual evaluation per vector: nothing to share);
 * the solver across ranks, as for adflow_gpu_gmres_solve; columns with different matrices or factors. */
#define ADFLOW_GPU_MAX_NVEC 32
int adflow_gpu_jacobian_mult_multi(int level, int transpose, int nvec, const double* X, long ldx, double* Y, long ldy, long n);
int adflow_gpu_jacobian_mult_multi_dev(int level, int transpose, int nvec, const double* d_X, long ldx, double* d_Y, long ldy, long n);
int adflow_gpu_pc_apply_multi(int level, int transpose, int nvec, const double* R, long ldr, double* Z, long ldz, long n);
int adflow_gpu_pc_apply_multi_dev(int level, int transpose, int nvec, const double* d_R, long ldr, double* d_Z, long ldz, long n);
int adflow_gpu_gmres_solve_multi(int level, int transpose, int nvec, const double* B, long ldb, double* X, long ldx, long n, int restart,
                                 int maxIts, double rtol, double atol, int useGuess, int* its, double* rnorm0, double* rnorm);
int adflow_gpu_gmres_solve_multi_dev(int level, int transpose, int nvec, const double* d_B, long ldb, double* d_X, long ldx, long n,
                                     int restart, int maxIts, double rtol, double atol, int useGuess, int* its, double* rnorm0,
                                     double* rnorm);

/* ---- the flow update of the approximate Newton-Krylov step, NKSolver::ANKStep (src/NKSolver/NKSolvers.F90:3629-4112) --------------
 * Everything acts on the level-1 blocks of the process.  Vectors: the layout of adflow_gpu_set_w_vec (block, k, j, i, variable
 * fastest) with nState variables per owned cell, n = nState x owned cells: nState = nw with ADFLOW_ANK_COUPLED, else 5 -- the flow
 * variables only, turbulence frozen, the reference's default ANK_coupled = .False. .  Host pointers, or device pointers for the _dev
 * forms, which honour adflow_gpu_set_async.
 *   adflow_gpu_ank_set_w   setWANK(wVec, 1, nState) (:2975-3011): w(i,j,k,1:nState) of the owned cells and nothing else.  Unlike setW
 *                          it does not clip the turbulence variable; nuTilde of a RANS block stays as it is without
 *                          ADFLOW_ANK_COUPLED.  Invalidates what adflow_gpu_set_w_vec invalidates.
 *   adflow_gpu_ank_get_r   setRVecANK (:2895-2933): dw / volRef of the flow variables, no turbResScale; with ADFLOW_ANK_COUPLED
 *                          setRVec (:1262-1329).
 *   adflow_gpu_ank_time_step   computeTimeStepMat / computeTimeStepBlock (:2041-2329) for ANK_charTimeStepType = 'None' (the default):
 *                          per owned cell of `level`  T = dtInv S,  dtInv = 1 / (cfl dtl volRef),  S = the state-to-conservative block
 *                          (ones on rho and rhoE, S(ivx..ivz, iRho) = u, v, w, S(ivx..ivz, ivx..ivz) = rho on the diagonal; with
 *                          ADFLOW_ANK_COUPLED also S(nt1, nt1) = turbResScale / turbCFLScale).  dtl is read as it stands on the device:
 *                          the caller refreshes it with adflow_gpu_time_step or ADFLOW_RES_UPDATE_INTERMED (see there).  No dense block
 *                          is stored: dtInv and rho, u, v, w of the state T was formed from (40 B per cell); products with T and the
 *                          shift of the diagonal are formed on the fly.  adflow_gpu_ank_download_time_step hands out the dense
 *                          blocks of block nn, (nState, nState, nx, ny, nz) column-major: timeStepMat for a host that wants it.
 *   adflow_gpu_ank_pc_setup    the ILU(0) of dRdwPre + timeStepMat (FormJacobianANK, :1996-1998): adflow_gpu_pc_setup with T added to
 *                          the diagonal blocks as the factorisation reads them.  It lands in the same factor slot:
 *                          adflow_gpu_pc_apply, _pc_info and _pc_release serve it unchanged.  Errors beside those of
 *                          adflow_gpu_pc_setup: no T, T's nState differs from the matrix's (a coupled T against an
 *                          ADFLOW_JAC_FROZEN_TURB matrix), T formed on another level.
 *   adflow_gpu_ank_set_base    formFunction_mf(wVec, baseRes) + MatMFFDSetBase (:3906-3908): sets the state from w (as
 *                          adflow_gpu_ank_set_w), evaluates the residual and keeps w and r0 = R(w) on the device.  flags:
 *                          ADFLOW_ANK_COUPLED plus ADFLOW_RES_DISS_APPROX, _VISC_APPROX, _UPWIND_FIRST_ORDER, passed to the residual
 *                          = blocketteRes(useDissApprox, useViscApprox, useTurbRes = ANK_coupled, useStoreWall = F) (:2500).  The
 *                          caller freezes the sensor first (adflow_gpu_reference_shock_sensor), as ANKStep:3859 does.
 *   adflow_gpu_ank_mult    y = (R(w + h v) - r0) / h + T v: what MatMFFD computes from FormFunction_mf (:2468-2538, R(u) + T u), the
 *                          linear part taken analytically instead of differenced.  h is PETSc's default MATMFFD_DS step:
 *                          s = w.v, d = |v|_1, q = |v|_2^2; |s| < umin d: s = +-umin d (the sign of s, + for zero);
 *                          h = errRel s / q, errRel = 1.490116119384766e-08, umin = 1e-6.  h is formed and read on the device and never
 *                          visits the host (adflow_gpu_ank_last_h downloads it, for tests): an application has no host
 *                          synchronisation of its own.  v = 0 gives y = 0; the host-pointer form then evaluates no residual, the
 *                          _dev form cannot know without a synchronisation and evaluates R(w).  v and y must differ.  AFTER A PRODUCT
 *                          THE DEVICE STATE IS THE PERTURBED ONE w + h v, as in the reference (physicalityCheckANK notes it,
 *                          :3043-3046): call adflow_gpu_ank_set_w before anything that reads the state.
 *   adflow_gpu_ank_solve   KSPSolve(ANK_KSP, rVec, deltaW) (:3912): the GMRES of adflow_gpu_gmres_solve with adflow_gpu_ank_mult as
 *                          operator and the factor slot as right preconditioner; starts from zero, never transposed.  Errors: those
 *                          of adflow_gpu_gmres_solve (more than one rank included), no base, no T, a factor whose nState differs.
 *   adflow_gpu_ank_physicality_check   physicalityCheckANK (:3013-3210, real mode; eps = 1e-25 of constants.F90): *lambda comes in as the
 *                          start value and goes out as the minimum over the cells of |w / (dw + eps)| physLSTol for density and
 *                          energy.  With ADFLOW_ANK_COUPLED the turbulence rule: the ratio (w / (dw + eps)) physLSTolTurb is signed; a
 *                          ratio below stepFactor stepMin does not limit the step, and if it is positive dw of that entry is
 *                          overwritten with w physLSTolTurb.  A NaN gives *lambda = 0.  More than one rank is an error: the
 *                          mpi_allreduce is the host's.  Synchronous (lambda goes to the host).
 * The rest of the step is the host's, on its device vectors: rVec = adflow_gpu_ank_get_r of the base state, deltaW from
 * adflow_gpu_ank_solve, lambda from adflow_gpu_ank_physicality_check, the `lambda < stepMin` rule, VecAXPY(wVec, -lambda, deltaW),
 * adflow_gpu_ank_set_w(wVec) + adflow_gpu_ank_unsteady_res for the backtracking, the CFL ramp; INTEGRATION.md has the call sites.
 * Lifetime: T, the base vectors and the sums are released by adflow_gpu_ank_release (*bytes, may be NULL: what was released),
 * adflow_gpu_block_release and adflow_gpu_release_all; adflow_gpu_release_workspace does not touch them.
 * approxSA: every entry that evaluates a residual takes ADFLOW_RES_APPROX_SA (and ADFLOW_RES_TURB_FIRST_ORDER) next to the three
 * approximate-flux flags; the matrices take ADFLOW_JAC_APPROX_SA.
 *
 * The turbulence KSP of the decoupled step, ANKTurbSolveKSP (:3337-3627): the same entries with ADFLOW_ANK_TURB, which excludes
 * ADFLOW_ANK_COUPLED and needs RANS.  Vectors carry nState = nt2 - nt1 + 1 = 1 entry per owned cell, nuTilde.
 *   adflow_gpu_ank_set_w   setWANK(wVecTurb, nt1, nt2) (:2975-3011): nuTilde of the owned cells, no clipping, nothing else.
 *   adflow_gpu_ank_get_r   setRVecANKTurb (:2935-2973): dw(itu1) / volRef turbResScale.
 *   adflow_gpu_ank_time_step   stores dtInv = 1 / (cfl dtl volRef) only, 8 B per cell; the diagonal is dtInv turbResScale /
 *                          turbCFLScale (FormJacobianANKTurb :2395-2406, FormFunction_mf_turb :2588-2594).  The flow T and the
 *                          turbulence T are kept side by side; the flag selects one on every entry.
 *                          adflow_gpu_ank_download_time_step_turb(nn, blocks, flags): with ADFLOW_ANK_TURB the turbulence T of block
 *                          nn, (1, 1, nx, ny, nz); with flags = 0 what adflow_gpu_ank_download_time_step hands out.
 *   adflow_gpu_ank_pc_setup    takes the turbulence T when the assembled matrix is an ADFLOW_JAC_TURB_ONLY one (nState = 1: the scalar
 *                          is added to the pivot, FormJacobianANKTurb), else the flow T; the errors are those above.
 *   adflow_gpu_ank_set_base / _mult / _solve   FormFunction_mf_turb (:2540-2612): blocketteRes(useFlowRes = F, useStoreWall = F) =
 *                          ADFLOW_RES_HALO | ADFLOW_RES_TURB with the turbulence boundary conditions and whalo2(1, nt1, nt2);
 *                          y = (R_t(w + h v) - r0) / h + T_t v with the same MATMFFD_DS h.  The state write re-forms the eddy
 *                          viscosity of the cell from rho, rlv and the new nuTilde (the arithmetic of computeEddyViscosity in the
 *                          closures) and nothing else: the flow variables do not move, so the pressure and the laminar viscosity
 *                          ON THE DEVICE MUST BE THOSE OF THE FLOW STATE (they are after any residual evaluation with closures or
 *                          any flow entry of this section).  Each kind keeps its own base; mult and solve act on the base set last, or on the
 *                          one adflow_gpu_ank_select_base(0 or ADFLOW_ANK_TURB) names (an error when that kind has none).
 *   adflow_gpu_ank_physicality_check   physicalityCheckANKTurb (:3212-3335): the signed-ratio rule above on the single entry, the
 *                          clipping of dw included; no density / energy rule.
 * The line search: adflow_gpu_ank_unsteady_res is computeUnsteadyResANK / computeUnsteadyResANKTurb (:2614-2786).  The state is the
 * one the caller set with adflow_gpu_ank_set_w (w - omega dW).  It evaluates blocketteRes(useTurbRes = ANK_coupled) -- with
 * ADFLOW_ANK_TURB blocketteRes(useFlowRes = F) -- closures, boundary conditions and whalo2 included, with the real fluxes unless the
 * approximate flags are passed, and writes r = setRVecANK / setRVec / setRVecANKTurb - omega T dW with the T of the matching kind as
 * stored (for the flow: of the state T was formed from, as timeStepMat is in the reference), and ||r||_2 to *norm: one pass over dw,
 * volRef, T and dW; partial sums per workgroup, added in a fixed order by one finishing workgroup, so the norm is the same from run
 * to run.  Synchronous because of norm; norm == NULL in the _dev form skips the reduction and honours adflow_gpu_set_async.  dw on
 * the device afterwards holds the steady residual (:2630-2633).  More than one rank with norm != NULL is an error.
 *
 * Out of scope: the Eisenstat-Walker, CFL-ramp and lag logic (the host's scalar code); ANK_useTurbDADI (adflow_gpu_sa_solve); the
 * Turkel and VLR time-step types; ANK_precondType = 'mg'; more than one rank; other turbulence models; ILU(k > 0), RCM and ASM
 * overlap, as above. */
enum { ADFLOW_ANK_COUPLED = 256u, ADFLOW_ANK_TURB = 512u };
int adflow_gpu_ank_set_w(const double* w, long n, unsigned flags);
int adflow_gpu_ank_set_w_dev(const double* d_w, long n, unsigned flags);
int adflow_gpu_ank_get_r(double* r, long n, unsigned flags);
int adflow_gpu_ank_get_r_dev(double* d_r, long n, unsigned flags);
int adflow_gpu_ank_time_step(int level, double cfl, double turbCFLScale, unsigned flags);
int adflow_gpu_ank_download_time_step(int nn, double* blocks);
int adflow_gpu_ank_download_time_step_turb(int nn, double* blocks, unsigned flags);
int adflow_gpu_ank_pc_setup(int level);
int adflow_gpu_ank_set_base(const double* w, long n, unsigned flags);
int adflow_gpu_ank_set_base_dev(const double* d_w, long n, unsigned flags);
int adflow_gpu_ank_mult(const double* v, double* y, long n);
int adflow_gpu_ank_mult_dev(const double* d_v, double* d_y, long n);
int adflow_gpu_ank_last_h(double* h);
int adflow_gpu_ank_select_base(unsigned flags);
int adflow_gpu_ank_solve(int level, const double* b, double* x, long n, int restart, int maxIts, double rtol, double atol, int* its,
                         double* rnorm0, double* rnorm);
int adflow_gpu_ank_solve_dev(int level, const double* d_b, double* d_x, long n, int restart, int maxIts, double rtol, double atol, int* its,
                             double* rnorm0, double* rnorm);
int adflow_gpu_ank_physicality_check(const double* w, double* dw, long n, unsigned flags, double physLSTol, double physLSTolTurb,
                                     double stepFactor, double stepMin, double* lambda);
int adflow_gpu_ank_physicality_check_dev(const double* d_w, double* d_dw, long n, unsigned flags, double physLSTol, double physLSTolTurb,
                                         double stepFactor, double stepMin, double* lambda);
int adflow_gpu_ank_unsteady_res(const double* dW, double omega, double* r, long n, unsigned flags, double* norm);
int adflow_gpu_ank_unsteady_res_dev(const double* d_dW, double omega, double* d_r, long n, unsigned flags, double* norm);
int adflow_gpu_ank_release(int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* ADFLOW_GPU_H */
