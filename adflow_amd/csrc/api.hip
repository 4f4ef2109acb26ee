// C-ABI entry points (include/adflow_gpu.h): block registry, HBM mirrors,
// host<->device transfers and the launch sequences of the hot path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <array>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "internal.h"
#include "flow_plan.h"
#include "pc_order.h"

extern int g_march_kch, g_viscous_tiled, g_inviscid_march, g_roe_march, g_sa_march;
int g_test_fault = 0;        // tuning "test_fault" (tests only): bit 0 = the hipGraph capture of a multigrid cycle reports failure, bit 1 = the
                             // split evaluation fails behind its fork -- the error paths must leave the library usable
int g_rvec_joint = 1;        // tuning "rvec_joint": the six entries of a cell of the matrix-free residual vector written by ONE kernel (KParams::rvecTurbFromDw)
int g_pc_fused = 1;          // tuning "pc_fused": first-order Roe + thin-layer viscous flux of the preconditioner matrix as ONE march (kernels_pc_march.hip), plain and dual
int g_xcd_tiles = 2;        // tuning "xcd_tiles": 0 = tiles in launch order, 1 = XCD x owns the x-th eighth of the launch, 2 = of every round

namespace {

std::string g_err;
int g_device = -1;
hipStream_t g_stream = nullptr;
// side streams of blocketteRes: the SA residual and the nodal gradients are independent of the inviscid kernel (which is bound by
// FP64 issue while they are bound by HBM): launched on their own queues they share the CUs with it (tuning "overlap")
hipStream_t g_streamB = nullptr, g_streamC = nullptr;
hipEvent_t g_evFork = nullptr, g_evB = nullptr, g_evC = nullptr, g_evB1 = nullptr;
hipStream_t g_streamX = nullptr;                 // the RCCL send / recv group of a halo exchange
hipEvent_t g_evPack = nullptr, g_evComm = nullptr;
int g_overlap = 1;
adflow_opts g_opts;
bool g_have_opts = false;
hipEvent_t g_events[64];
bool g_events_ready = false;
bool g_async = false;   // adflow_gpu_set_async: entry points enqueue only

int fail(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct DevArr {
    double* base = nullptr;   // hipMalloc pointer
    int ncomp = 0;
};

struct Block {
    adflow_block_desc d;
    BlkView v;
    long boxsize = 0;         // ldi*(jb+1)*(kb+1)
    std::vector<void*> allocs;
    bool geom_uploaded = false;
    bool normals_from_x_ok = true;     // the uploaded sI / sJ / sK equal metric_block(x): the kernels may re-form them from the nodes
    unsigned geom_is_host = 0;         // bit 0..3: the device copy of x / sI / sJ / sK IS the descriptor's host array (set by an upload from
                                       // the registered pointer, cleared by an upload from any other buffer): normals_match_nodes reads the
                                       // HOST arrays, so it speaks for the device only when all four bits are set (round-4 advisor finding)
    bool face_vectors_valid = false;   // dI/dJ/dK derived from x
    bool ss_valid = false;    // entropy sensor variable matches the current state
    bool etot_consistent = false;   // owned-cell rhoE already equals computeEtotBlock(p, rho, v)
    std::vector<BcFaceDev> bc;      // boundary subfaces (device BCData), first nViscBocos = viscous walls
    std::vector<void*> bc_allocs;   // device copies of the BCData members: replaced at every bc_register
    int nViscBocos = 0;
    bool tau_stored = false;        // a storing evaluation has written viscSubface%tau / %q since the subfaces were registered
    // adflow_gpu_bc_set_families: BCData(mm)%famID and the device copy of %iblank (NULL = all ones) of every subface; empty = family 0
    std::vector<int> famID;
    std::vector<const signed char*> faceBlank;
    std::vector<void*> fam_allocs;
    // coloured finite-difference Jacobian (adflow_gpu_fd_jacobian): reference state / residual, stencil blocks
    double *wref = nullptr, *dwref = nullptr, *jac = nullptr, *snap = nullptr;
    void *jac_raw = nullptr, *snap_raw = nullptr;
    int jac_ncomp = 0, snap_ncomp = 0;
    // wall association of updateWallDistancesQuickly: surfNodeIndices (4,nx,ny,nz), uv (2,nx,ny,nz)
    int* wd_ind = nullptr;
    double* wd_uv = nullptr;
    int wd_max_node = 0;               // largest 1-based surface node the association refers to
};

typedef std::tuple<int, int, int> Key;   // (level, sps, nn): iteration order = level, sps, nn
std::map<Key, Block*> g_blocks;

struct CommList {          // device index lists of one message / of the local copies
    int n = 0;
    int *blkA = nullptr, *blkB = nullptr;     // donor/halo block slots (pack/unpack use blkA only)
    long *offA = nullptr, *offB = nullptr;
    int peer = -1;
    double* buf = nullptr;                    // device message buffer (11 variables max)
};

struct CommPattern {
    bool present = false;
    CommList local;
    std::vector<CommList> sends, recvs;
    // host copies of the index triples until the block table is known
    std::vector<int32_t> h_donorBlock, h_donorIdx, h_haloBlock, h_haloIdx;
    std::vector<int32_t> h_sendProc, h_nsendCum, h_sendBlock, h_sendIdx;
    std::vector<int32_t> h_recvProc, h_nrecvCum, h_recvBlock, h_recvIdx;
    // periodic transformations (periodicDataType): halos they apply to
    struct Periodic {
        double rotMatrix[9], rotCenter[3], translation[3];
        std::vector<int32_t> h_block, h_idx;
        CommList list;
    };
    std::vector<Periodic> periodic;
    bool built = false;
    // the exchange in reverse (adflow_gpu_jacobian_mult, transposed): donor-sorted accumulation lists, [0] the same-process pairs,
    // [1 + i] the message that comes back over send list i; built at the first transposed product
    std::vector<JmAccList> acc;
    bool accBuilt = false;
};

struct ActRegion {       // one actuator region (actuatorRegionData.F90); the cell list addresses level-1 blocks
    std::vector<int32_t> h_block, h_idx;      // h_idx (n,3) column-major as make_list expects
    double force[3], heat, volume, relaxStart, relaxEnd;
    CommList list;
    bool built = false;
};
std::vector<ActRegion> g_act;

std::map<std::pair<int, int>, CommPattern> g_comm;   // (level, nLayers)
double* g_rvec_target = nullptr;     // residual vector the kernels of the evaluation in flight write (nk_residual_dev)
int g_rvec_done = 0;                  // bit 0: flow entries written, bit 1: turbulence entry written
int g_snap_done = 0;                  // the same for the snapshot entries of a coloured Jacobian evaluation (KParams::snapTab)
long g_pc_topo_gen = 0;      // bumped when a block or a comm pattern is registered or released: the pattern tables of a factor over the level
                             // (adflow_gpu_pc_set_level_fill) are kept across setups while it stands
long g_state_gen = 0;        // bumped by every call that changes what a multigrid cycle enqueues (options, tuning, blocks, patterns, subfaces)
int g_split_eval = 1;       // tuning "split_eval": whalo2 + blocketteRes with the halo-free tiles inside the exchange: 1 = when the pattern has messages, 2 = always, 0 = never
int g_mg_graph = 1;         // tuning "mg_graph": a repeated adflow_gpu_mg_cycle is captured once into a hipGraph and replayed
int g_comm_self = 0;        // tuning "comm_self": same-process interfaces through pack / RCCL send+recv to self / unpack
int g_self_rank = 0;        // rank of this process in the RCCL communicator
std::map<int, BlkView*> g_tab;                        // level -> device table indexed by nn
std::map<int, int> g_tab_size;
std::map<int, std::pair<int4*, int>> g_tiles;          // level -> XCD-ordered tile table of the marching kernel
std::map<int, std::pair<int4*, int>> g_gf_tiles;       // level -> round-fitted chunk table of k_visc_gf
std::map<int, std::pair<int4*, int>> g_gf_tiles_int, g_gf_tiles_bnd;   // the same chunks: those that read no halo cell / the others
std::map<int, std::pair<int4*, int>> g_sa_tiles, g_sa_tiles_int, g_sa_tiles_bnd;   // the same three for k_sa_march
int g_num_cus = 0;
int g_gf_nofit = 0;         // tuning gf_cus = -1 (tests): chunks of march_kch planes instead of the round fit
int g_phase_base = 0;                                    // tuning "phase_events": first of 8 event slots, 0 = off
bool g_use_march = true;                               // tuning: adflow_gpu_set_tuning("euler_march", 0|1)
adflow_bc_callback g_bc_callback = nullptr;
adflow_bc_callback g_turb_bc_callback = nullptr;
double* g_norm_dev = nullptr;
int* g_floor_flag_dev = nullptr;      // raised by k_set_w_closures_level when a pressure hit its floor (FormFunction_mf)
int g_dadi_upd = 1;                  // tuning "dadi_upd": the D-ADI state update inside the k sweep's back substitution
int g_etot_flag_level = 0;            // > 0: the next whalo2 close on that level recomputes the owned energy only if the floor flag is up

void free_list(CommList& l)
{
    if (l.blkA) (void)hipFree(l.blkA);
    if (l.blkB) (void)hipFree(l.blkB);
    if (l.offA) (void)hipFree(l.offA);
    if (l.offB) (void)hipFree(l.offB);
    if (l.buf) (void)hipFree(l.buf);
    l = CommList();
}

void free_acc_list(JmAccList& a)
{
    if (a.tBlk) (void)hipFree(a.tBlk);
    if (a.tOff) (void)hipFree(a.tOff);
    if (a.seg) (void)hipFree(a.seg);
    if (a.sBlk) (void)hipFree(a.sBlk);
    if (a.sOff) (void)hipFree(a.sOff);
    a = JmAccList();
}

// device lists of a pattern: rebuilt from the host copies at the next exchange
void drop_comm_lists(CommPattern& cp)
{
    for (auto& a : cp.acc) free_acc_list(a);
    cp.acc.clear();
    cp.accBuilt = false;
    free_list(cp.local);
    for (auto& l : cp.sends) free_list(l);
    for (auto& l : cp.recvs) free_list(l);
    for (auto& pd : cp.periodic) free_list(pd.list);
    cp.sends.clear();
    cp.recvs.clear();
    cp.built = false;
}

void invalidate_comm_level(int level)
{
    ++g_state_gen;
    if (level == 1)
        for (auto& r : g_act) r.built = false;      // cell offsets depend on the registered blocks
    for (auto& kv : g_comm)
        if (kv.first.first == level) drop_comm_lists(kv.second);
    auto it = g_tab.find(level);
    if (it != g_tab.end()) {
        (void)hipFree(it->second);
        g_tab.erase(it);
    }
    auto jt = g_tiles.find(level);
    if (jt != g_tiles.end()) {
        (void)hipFree(jt->second.first);
        g_tiles.erase(jt);
    }
    for (auto* mp : {&g_gf_tiles, &g_gf_tiles_int, &g_gf_tiles_bnd, &g_sa_tiles, &g_sa_tiles_int, &g_sa_tiles_bnd}) {
        jt = mp->find(level);
        if (jt != mp->end()) {
            (void)hipFree(jt->second.first);
            mp->erase(jt);
        }
    }
}


int ensure_table(int level);
int res_averaging_level(int level, const KParams& kp, double scaleDtl = 0.0);
int time_step_level(int level, const KParams& kp);
struct LevelTab { const BlkView* tab; int n, nx, ny, nz; };
int level_tab(int level, LevelTab* t);
int ensure_tiles(int level);
int ensure_gf_tiles(int level);
int ensure_sa_tiles(int level);
int build_comm(int level, int nLayers, CommPattern** out);
int halo_mask(int varStart, int varEnd, int commPressure, int commVisc, unsigned* mask, int* nvar);
int make_list(int level, const int32_t* blk, const int32_t* idx, int ld, int first, int n, int** d_blk, long** d_off);

Block* find_block(int nn, int level, int sps)
{
    auto it = g_blocks.find(Key(level, sps, nn));
    return it == g_blocks.end() ? nullptr : it->second;
}

int alloc_arr(Block* b, double** p, int ncomp)
{
    size_t bytes = (size_t)b->v.nbox * ncomp * sizeof(double) + 256;
    void* raw = nullptr;
    HIPCHK(hipMalloc(&raw, bytes));
    HIPCHK(hipMemsetAsync(raw, 0, bytes, g_stream));
    b->allocs.push_back(raw);
    *p = (double*)raw + ADF_PAD0;
    return 0;
}

// pinned staging buffer (grown on demand) for host <-> device box transfers
double* g_stage = nullptr;
size_t g_stage_elems = 0;

int stage_reserve(size_t elems)
{
    if (elems <= g_stage_elems) return 0;
    if (g_stage) (void)hipHostFree(g_stage);
    g_stage = nullptr;
    g_stage_elems = 0;
    HIPCHK(hipHostMalloc((void**)&g_stage, elems * sizeof(double), hipHostMallocDefault));
    g_stage_elems = elems;
    return 0;
}

// host sub-box (lo..lo+n-1 in each direction, column-major, ncomp components)
// <-> device box component(s).  The host side is the reference's pageable
// Fortran array; rows are (un)packed through one pinned buffer holding the
// k-slab range of the padded device box, moved with a single DMA per component.
int copy_box(Block* b, double* dev, const double* host_c, int ncomp, int lo_i, int n_i, int lo_j, int n_j, int lo_k, int n_k,
             bool to_device)
{
    if (!host_c) return 0;
    double* host = const_cast<double*>(host_c);
    const BlkView& v = b->v;
    const size_t slab = (size_t)v.ldk * n_k;            // padded elements covering k = lo_k .. lo_k+n_k-1
    if (stage_reserve(slab)) return 1;
    for (int c = 0; c < ncomp; ++c) {
        double* dptr = dev + (size_t)c * v.nbox + v.idx(0, 0, lo_k);
        double* hcomp = host + (size_t)c * n_i * n_j * n_k;
        if (to_device) {
            // read-modify-write of the slab keeps device values outside the sub-box
            const bool partial = (lo_i != 0 || lo_j != 0 || n_i != v.ib + 1 || n_j != v.jb + 1);
            if (partial) {
                HIPCHK(hipMemcpyAsync(g_stage, dptr, slab * 8, hipMemcpyDeviceToHost, g_stream));
                HIPCHK(hipStreamSynchronize(g_stream));
            }
            for (int k = 0; k < n_k; ++k)
                for (int j = 0; j < n_j; ++j)
                    memcpy(g_stage + (size_t)k * v.ldk + (size_t)(j + lo_j) * v.ldi + lo_i,
                           hcomp + ((size_t)k * n_j + j) * n_i, (size_t)n_i * 8);
            HIPCHK(hipMemcpyAsync(dptr, g_stage, slab * 8, hipMemcpyHostToDevice, g_stream));
            HIPCHK(hipStreamSynchronize(g_stream));
        } else {
            HIPCHK(hipMemcpyAsync(g_stage, dptr, slab * 8, hipMemcpyDeviceToHost, g_stream));
            HIPCHK(hipStreamSynchronize(g_stream));
            for (int k = 0; k < n_k; ++k)
                for (int j = 0; j < n_j; ++j)
                    memcpy(hcomp + ((size_t)k * n_j + j) * n_i,
                           g_stage + (size_t)k * v.ldk + (size_t)(j + lo_j) * v.ldi + lo_i, (size_t)n_i * 8);
        }
    }
    return 0;
}

int g_lumped = 0;       // inputDiscretization::lumpedDiss while a preconditioner matrix is assembled
int g_metric_from_x = 5;   // tuning "metric_from_x": bit 0 the SA march, bit 2 the time-step kernel re-form the face normals from the node coordinates.
                           // (k_visc_gf and k_roe_march keep the stored normals: the node form costs more registers than either has --
                           // profiles/r06_a_xn_2wg_*, r02_ba_variants.txt)

// the snapshot request of a Jacobian assembly (KParams::snapTab): set around the coloured evaluations of adflow_gpu_fd_jacobian
struct SnapReq { bool on = false; SnapSlot* dev = nullptr; int devSlots = 0; int level = 0, col = 0, l0 = 0, n = 0; double turbScale = 1.0; };
static SnapReq g_snapreq;
int g_jac_snap = 1;         // tuning "jac_snap": the marching kernels of the preconditioner matrix write the snapshots themselves (0: k_fd_snap / k_ad_snap)

KParams make_kparams(int level, double rFil, int fwMode)
{
    const adflow_opts& o = g_opts;
    KParams k;
    memset(&k, 0, sizeof k);
    k.equations = o.equations;
    k.spaceDiscr = (level == 1) ? o.spaceDiscr : o.spaceDiscrCoarse;
    k.limiter = o.limiter;
    k.orderTurb = o.orderTurb;
    k.turbProd = o.turbProd;
    k.viscous = (o.equations == ADFLOW_NS || o.equations == ADFLOW_RANS);
    k.eddyModel = (o.equations == ADFLOW_RANS);
    k.dirScaling = o.dirScaling;
    k.lumpedDiss = g_lumped;
    k.metricFromX = g_metric_from_x;
    if (k.metricFromX)
        for (auto& kv : g_blocks)
            if (std::get<0>(kv.first) == level && !kv.second->normals_from_x_ok) { k.metricFromX = 0; break; }
    k.sigma = o.sigma;
    k.useQCR = o.useQCR;
    k.useRotationSA = o.useRotationSA;
    k.useft2SA = o.useft2SA;
    k.fineGrid = (level == o.groundLevel);
    k.groundLevelIsOne = (o.groundLevel == 1);
    k.doScaling = (o.dirScaling && level <= o.groundLevel);
    k.coarseInit = (level != o.groundLevel);
    k.fwMode = fwMode;
    k.updateEddy = (level <= o.groundLevel);
    k.rFil = rFil;
    k.sfil = 1.0 - rFil;
    k.vis2 = o.vis2; k.vis4 = o.vis4; k.vis2Coarse = o.vis2Coarse; k.adis = o.adis;
    k.acousticScaleFactor = o.acousticScaleFactor; k.kappaCoef = o.kappaCoef;
    k.gammaConstant = o.gammaConstant; k.gammaInf = o.gammaInf; k.pInf = o.pInf; k.pInfCorr = o.pInfCorr; k.rhoInf = o.rhoInf; k.RGas = o.RGas;
    k.muRef = o.muRef; k.TRef = o.TRef; k.timeRef = o.timeRef;
    k.prandtl = o.prandtl; k.prandtlTurb = o.prandtlTurb;
    k.SSuthDim = o.SSuthDim; k.muSuthDim = o.muSuthDim; k.TSuthDim = o.TSuthDim;
    k.sa_k = o.SAKappa; k.sa_cb1 = o.SAcb1; k.sa_cb2 = o.SAcb2; k.sa_cb3 = o.SAsigma; k.sa_cv1 = o.SAcv1;
    k.sa_cw1 = o.SAcw1; k.sa_cw2 = o.SAcw2; k.sa_cw3 = o.SAcw3; k.sa_ct3 = o.SAct3; k.sa_ct4 = o.SAct4;
    k.sa_crot = o.SAcrot;
    k.sa_qqFactor = (o.turbRelax == 2) ? 1.0 + (1.0 - o.alfaTurb) / o.alfaTurb : 1.0;
    k.sa_updFactor = (o.turbRelax == 1) ? o.alfaTurb : 1.0;
    k.cfl = (level == 1) ? o.cfl : o.cflCoarse;
    k.cflLimit = o.cflLimit; k.smoop = o.smoop; k.fcoll = o.fcoll; k.turbResScale = o.turbResScale;
    for (int i = 0; i < 10; ++i) k.wInf[i] = o.wInf[i];
    if (g_snapreq.on && level == g_snapreq.level) {
        k.snapTab = g_snapreq.dev; k.snapCol = g_snapreq.col; k.snapL0 = g_snapreq.l0; k.snapN = g_snapreq.n;
        k.snapTurbScale = g_snapreq.turbScale;
    }
    return k;
}

int need_ready(void)
{
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    if (!g_have_opts) return fail("adflow_gpu_set_options has not been called");
    return 0;
}

template <typename Fn>
int for_level(int level, Fn fn)
{
    bool any = false;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level) continue;
        any = true;
        int rc = fn(kv.second);
        if (rc) return rc;
    }
    if (!any) return fail("no block registered on level %d", level);
    return 0;
}

}  // namespace
// instrumentation of blocketteRes (tuning "phase_events" = first event slot): marks 0 entry, 1 closures / BCs / halos done,
// 2 time step, 3 SA residual, 4 inviscid fluxes, 5 nodal gradients, 6 viscous fluxes + sources (end); with the viscous march in
// front of the Roe march (tuning visc_first): 4 nodal gradients, 5 viscous fluxes, 6 inviscid fluxes + sources
void adf_phase_mark(int i)
{
    static unsigned hit = 0;
    if (g_phase_base <= 0 || !g_stream) return;
    if (i == 0) hit = 0;
    if (i == 6)      // phases this configuration does not have (no viscous part, fused kernels): zero-length, closed here
        for (int m = 1; m < 6; ++m)
            if (!(hit & (1u << m))) (void)hipEventRecord(g_events[g_phase_base + m], g_stream);
    hit |= 1u << i;
    (void)hipEventRecord(g_events[g_phase_base + i], g_stream);
}
namespace {
inline void phase_mark(int i) { adf_phase_mark(i); }

int sync_and_check(void)
{
    HIPCHK(hipGetLastError());
    if (!g_async) HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

}  // namespace

extern "C" {

const char* adflow_gpu_last_error(void) { return g_err.c_str(); }

int adflow_gpu_init(int device_ordinal)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail("no HIP device visible: the MI355X engine has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= n) return fail("device ordinal %d out of range (%d devices)", device_ordinal, n);
    HIPCHK(hipSetDevice(device_ordinal));
    if (!g_stream) HIPCHK(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    if (!g_streamB) {
        HIPCHK(hipStreamCreateWithFlags(&g_streamB, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&g_streamC, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&g_evFork)); HIPCHK(hipEventCreate(&g_evB)); HIPCHK(hipEventCreate(&g_evC)); HIPCHK(hipEventCreate(&g_evB1));
        HIPCHK(hipStreamCreateWithFlags(&g_streamX, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&g_evPack, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&g_evComm, hipEventDisableTiming));
    }
    if (!g_events_ready) {
        for (int i = 0; i < 64; ++i) HIPCHK(hipEventCreate(&g_events[i]));
        g_events_ready = true;
    }
    g_device = device_ordinal;
    return 0;
}

int adflow_gpu_device_name(char* buf, int len)
{
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, g_device));
    snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return 0;
}

static void free_side_buffers(void);

int adflow_gpu_finalize(void)
{
    // device tables, tile tables, communication patterns, boundary plans and every block: the same path as release_all, so
    // that an init after a finalize starts from an empty registry
    if (g_device >= 0) (void)adflow_gpu_release_all();
    free_side_buffers();
    if (g_events_ready) {
        for (int i = 0; i < 64; ++i) (void)hipEventDestroy(g_events[i]);
        g_events_ready = false;
    }
    if (g_stage) {
        (void)hipHostFree(g_stage);
        g_stage = nullptr;
        g_stage_elems = 0;
    }
    if (g_streamB) {
        (void)hipStreamDestroy(g_streamB); (void)hipStreamDestroy(g_streamC); (void)hipStreamDestroy(g_streamX);
        (void)hipEventDestroy(g_evFork); (void)hipEventDestroy(g_evB); (void)hipEventDestroy(g_evC); (void)hipEventDestroy(g_evB1);
        (void)hipEventDestroy(g_evPack); (void)hipEventDestroy(g_evComm);
        g_streamB = g_streamC = g_streamX = nullptr;
    }
    if (g_stream) {
        (void)hipStreamDestroy(g_stream);
        g_stream = nullptr;
    }
    g_device = -1;
    g_have_opts = false;
    return 0;
}

int adflow_gpu_set_options(const adflow_opts* o)
{
    if (!o) return fail("null options");
    if (o->equations < ADFLOW_EULER || o->equations > ADFLOW_RANS) return fail("equations=%d not supported", o->equations);
    if (o->nRKStages < 1 || o->nRKStages > ADFLOW_MAX_RK_STAGES) return fail("nRKStages=%d out of range", o->nRKStages);
    if (o->unsupported)
        return fail("configuration outside the GPU path:%s%s%s%s (this library computes the steady, constant-cp, 1-to-1 multiblock residual only)",
                    (o->unsupported & 1) ? " unsteady / time-spectral equationMode;" : "", (o->unsupported & 2) ? " cpModel /= cpConstant;" : "",
                    (o->unsupported & 4) ? " wall functions;" : "", (o->unsupported & 8) ? " overset blocks;" : "");
    if (o->equations == ADFLOW_RANS && o->turbModel != 2)   // spalartAllmaras (constants.F90)
        return fail("turbModel=%d not supported (Spalart-Allmaras only)", o->turbModel);
    if (o->equations == ADFLOW_RANS && o->turbProd != ADFLOW_TURBPROD_STRAIN && o->turbProd != ADFLOW_TURBPROD_VORTICITY)   // sa.F90:136-139 stops
        return fail("turbProd=%d not supported with Spalart-Allmaras (strain or vorticity; the reference stops for katoLaunder)", o->turbProd);
    if (memcmp(&g_opts, o, sizeof g_opts) != 0) ++g_state_gen;
    g_opts = *o;
    g_have_opts = true;
    return 0;
}

int adflow_gpu_block_register(int nn, int level, int sps, const adflow_block_desc* d)
{
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    if (!d) return fail("null block descriptor");
    if (d->nx < 1 || d->ny < 1 || d->nz < 1) return fail("block %d: bad dimensions %d %d %d", nn, d->nx, d->ny, d->nz);
    if (d->nw != 5 && d->nw != 6) return fail("block %d: nw=%d not supported (5, or 6 with SA)", nn, d->nw);
    if (find_block(nn, level, sps)) return fail("block (%d,%d,%d) already registered", nn, level, sps);
    // the level-batched kernels hold one spectral instance: a second one would silently keep stale dw / w
    if (sps != 1) return fail("block (%d,%d,%d): only sps = 1 (steady, one spectral instance) is supported", nn, level, sps);
    Block* b = new Block;
    b->d = *d;
    BlkView& v = b->v;
    memset(&v, 0, sizeof v);
    v.nx = d->nx; v.ny = d->ny; v.nz = d->nz; v.nw = d->nw;
    v.il = v.nx + 1; v.jl = v.ny + 1; v.kl = v.nz + 1;
    v.ie = v.nx + 2; v.je = v.ny + 2; v.ke = v.nz + 2;
    v.ib = v.nx + 3; v.jb = v.ny + 3; v.kb = v.nz + 3;
    v.ldi = ((v.ib + 1 + 15) / 16) * 16;
    v.ldk = v.ldi * (v.jb + 1);
    v.mfact = d->rightHanded ? 0.5 : -0.5;
    b->boxsize = (long)v.ldk * (v.kb + 1);
    v.nbox = ((b->boxsize + 15) / 16) * 16 + 16;
    int rc = 0;
    rc |= alloc_arr(b, &v.w, v.nw);
    rc |= alloc_arr(b, &v.p, 1);
    rc |= alloc_arr(b, &v.gamma, 1);
    rc |= alloc_arr(b, &v.rlv, 1);
    rc |= alloc_arr(b, &v.rev, 1);
    rc |= alloc_arr(b, &v.x, 3);
    rc |= alloc_arr(b, &v.sI, 3);
    rc |= alloc_arr(b, &v.sJ, 3);
    rc |= alloc_arr(b, &v.sK, 3);
    rc |= alloc_arr(b, &v.vol, 1);
    rc |= alloc_arr(b, &v.volRef, 1);
    rc |= alloc_arr(b, &v.d2wall, 1);
    if (d->addGridVelocities) {
        if (!(d->sFaceI && d->sFaceJ && d->sFaceK)) return fail("block (%d,%d,%d): addGridVelocities without sFaceI/J/K", nn, level, sps);
        rc |= alloc_arr(b, &v.sFace, 3);
    }
    v.moving = d->blockIsMoving ? 1 : 0;
    for (int m = 0; m < 3; ++m) v.rot[m] = d->rotRate[m];
    rc |= alloc_arr(b, &v.dI, 3);
    rc |= alloc_arr(b, &v.dJ, 3);
    rc |= alloc_arr(b, &v.dK, 3);
    rc |= alloc_arr(b, &v.xc, 3);
    rc |= alloc_arr(b, &v.dw, v.nw);
    rc |= alloc_arr(b, &v.fw, 5);
    rc |= alloc_arr(b, &v.dtl, 1);
    rc |= alloc_arr(b, &v.radI, 1);
    rc |= alloc_arr(b, &v.radJ, 1);
    rc |= alloc_arr(b, &v.radK, 1);
    rc |= alloc_arr(b, &v.ss, 1);
    rc |= alloc_arr(b, &v.aa, 1);
    rc |= alloc_arr(b, &v.grad, 12);
    rc |= alloc_arr(b, &v.scratch, 10);
    rc |= alloc_arr(b, &v.wn, 5);
    rc |= alloc_arr(b, &v.pn, 1);
    rc |= alloc_arr(b, &v.w1, 5);
    rc |= alloc_arr(b, &v.p1, 1);
    rc |= alloc_arr(b, &v.wr, 5);
    if (rc) return rc;
    {
        void* raw = nullptr;
        HIPCHK(hipMalloc(&raw, (size_t)v.nbox + 256));
        HIPCHK(hipMemsetAsync(raw, 0, (size_t)v.nbox + 256, g_stream));
        b->allocs.push_back(raw);
        v.flags = (uint8_t*)raw + 16;
    }
    // multigrid maps: small index arrays, re-laid out as [2*m + q]
    {
        auto up_pair = [&](const int32_t* h, int lo, int n, int** dev) -> int {
            *dev = nullptr;
            if (!h) return 0;
            std::vector<int> t((size_t)2 * (lo + n + 1), 0);
            for (int m = 0; m < n; ++m)
                for (int q = 0; q < 2; ++q) t[(size_t)2 * (lo + m) + q] = h[(size_t)m + (size_t)n * q];
            void* raw = nullptr;
            HIPCHK(hipMalloc(&raw, sizeof(int) * t.size()));
            HIPCHK(hipMemcpy(raw, t.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice));
            b->allocs.push_back(raw);
            *dev = (int*)raw;
            return 0;
        };
        auto up_w = [&](const double* h, int lo, int n, double** dev) -> int {
            *dev = nullptr;
            if (!h) return 0;
            std::vector<double> t((size_t)(lo + n + 1), 0.0);
            for (int m = 0; m < n; ++m) t[(size_t)lo + m] = h[m];
            void* raw = nullptr;
            HIPCHK(hipMalloc(&raw, sizeof(double) * t.size()));
            HIPCHK(hipMemcpy(raw, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
            b->allocs.push_back(raw);
            *dev = (double*)raw;
            return 0;
        };
        if (up_pair(d->mgIFine, 1, v.ie, &v.mgIFine) || up_pair(d->mgJFine, 1, v.je, &v.mgJFine) ||
            up_pair(d->mgKFine, 1, v.ke, &v.mgKFine) || up_w(d->mgIWeight, 2, v.nx, &v.mgIWeight) ||
            up_w(d->mgJWeight, 2, v.ny, &v.mgJWeight) || up_w(d->mgKWeight, 2, v.nz, &v.mgKWeight) ||
            up_pair(d->mgICoarse, 2, v.nx, &v.mgICoarse) || up_pair(d->mgJCoarse, 2, v.ny, &v.mgJCoarse) ||
            up_pair(d->mgKCoarse, 2, v.nz, &v.mgKCoarse))
            return 1;
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    g_blocks[Key(level, sps, nn)] = b;
    ++g_pc_topo_gen;
    invalidate_comm_level(level);
    return 0;
}

static void bc_plan_drop(int level);
static void bc_plan_drop_all();
static void ad_cache_drop();      // the cached dual arrays of the forward-mode assembly refer to the blocks
static int64_t jm_release();      // ... and so do the scratch arrays of the matrix products (adflow_gpu_jacobian_mult)
static int64_t pc_release_all();  // ... and the block ILU(0) factors of both slots (adflow_gpu_pc_setup, adflow_gpu_pc_select)
static int64_t ank_release();     // ... and the pseudo-time term, base vectors and sums of the ANK operator (adflow_gpu_ank_*)
static int64_t wi_drop(int level);   // ... and the buffers of the surface integration of a level (adflow_gpu_wall_integrate)
static int64_t wi_drop_all();
static bool g_jac_valid = false; // adflow_gpu_fd_jacobian left a matrix on the blocks of level g_jac_level
static int g_jac_level = 0;

int adflow_gpu_block_release(int nn, int level, int sps)
{
    auto it = g_blocks.find(Key(level, sps, nn));
    if (it == g_blocks.end()) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    bc_plan_drop(level);
    ad_cache_drop();
    (void)jm_release();
    (void)pc_release_all();
    (void)ank_release();
    for (void* p : it->second->allocs) (void)hipFree(p);
    if (it->second->jac_raw) (void)hipFree(it->second->jac_raw);
    if (it->second->snap_raw) (void)hipFree(it->second->snap_raw);
    for (void* p : it->second->bc_allocs) (void)hipFree(p);
    for (void* p : it->second->fam_allocs) (void)hipFree(p);
    delete it->second;
    g_blocks.erase(it);
    ++g_pc_topo_gen;
    invalidate_comm_level(level);
    return 0;
}

int adflow_gpu_release_all(void)
{
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    bc_plan_drop_all();
    ad_cache_drop();
    (void)jm_release();
    (void)pc_release_all();
    (void)ank_release();
    for (auto& kv : g_blocks) {
        for (void* p : kv.second->allocs) (void)hipFree(p);
        if (kv.second->jac_raw) (void)hipFree(kv.second->jac_raw);
        if (kv.second->snap_raw) (void)hipFree(kv.second->snap_raw);
        for (void* p : kv.second->bc_allocs) (void)hipFree(p);
        for (void* p : kv.second->fam_allocs) (void)hipFree(p);
        delete kv.second;
    }
    g_blocks.clear();
    ++g_pc_topo_gen;
    g_jac_valid = false;          // the stencil blocks went with the blocks
    {
        std::vector<int> levels;
        for (auto& kv : g_tab) levels.push_back(kv.first);
        for (int l : levels) invalidate_comm_level(l);
        g_comm.clear();
    }
    return 0;
}

// The marching kernels may re-form face normals from the node coordinates (tuning metric_from_x).  That is only the same
// computation if the host's sI / sJ / sK ARE metric_block(x) (adjointExtra.F90:176-268), which holds for every mesh the reference
// builds; a sample of faces of each array is checked against the cross products at upload, and a block that fails keeps the
// level on the stored normals instead of silently evaluating a different geometry.
static bool normals_match_nodes(const Block* b)
{
    const adflow_block_desc& d = b->d;
    const BlkView& v = b->v;
    if (!d.x || !d.sI || !d.sJ || !d.sK) return false;
    const double fact = d.rightHanded ? 0.5 : -0.5;
    const size_t nxn = (size_t)v.ie + 1, nyn = (size_t)v.je + 1, nzn = (size_t)v.ke + 1;        // x(0:ie, 0:je, 0:ke, 3)
    auto X = [&](int i, int j, int k, int q) { return d.x[(size_t)i + nxn * ((size_t)j + nyn * ((size_t)k + nzn * q))]; };
    auto cross = [&](const double p1[3], const double p2[3], const double q1[3], const double q2[3], double s[3]) {
        const double a[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]}, c[3] = {q1[0] - q2[0], q1[1] - q2[1], q1[2] - q2[2]};
        s[0] = fact * (a[1] * c[2] - a[2] * c[1]); s[1] = fact * (a[2] * c[0] - a[0] * c[2]); s[2] = fact * (a[0] * c[1] - a[1] * c[0]);
    };
    auto node = [&](int i, int j, int k, double p[3]) { for (int q = 0; q < 3; ++q) p[q] = X(i, j, k, q); };
    double worst = 0.0, scale = 0.0;
    const int ns = 5;
    for (int a = 0; a < ns; ++a)
        for (int c = 0; c < ns; ++c)
            for (int e = 0; e < ns; ++e) {
                // sample points spread over the index ranges incl. the first and last faces
                const int i = 1 + (int)((long)(v.ie - 1) * a / (ns - 1)), j = 1 + (int)((long)(v.je - 1) * c / (ns - 1)),
                          k = 1 + (int)((long)(v.ke - 1) * e / (ns - 1));
                double n11[3], n10[3], n01[3], n00[3], s[3];
                // sI(i, j, k), i = 0..ie, j = 1..je, k = 1..ke: nodes (i, j-1..j, k-1..k)
                node(i, j, k - 1, n11); node(i, j - 1, k, n10); node(i, j, k, n01); node(i, j - 1, k - 1, n00);
                cross(n11, n10, n01, n00, s);
                for (int q = 0; q < 3; ++q) {
                    const double h = d.sI[(size_t)i + nxn * ((size_t)(j - 1) + (size_t)v.je * ((size_t)(k - 1) + (size_t)v.ke * q))];
                    worst = std::max(worst, fabs(h - s[q])); scale = std::max(scale, fabs(h));
                }
                // sJ(i, j, k), i = 1..ie, j = 0..je, k = 1..ke: v1 = x(i,j,n) - x(l,j,k) ; v2 = x(l,j,n) - x(i,j,k)
                node(i, j, k - 1, n11); node(i - 1, j, k, n10); node(i - 1, j, k - 1, n01); node(i, j, k, n00);
                cross(n11, n10, n01, n00, s);
                for (int q = 0; q < 3; ++q) {
                    const double h = d.sJ[(size_t)(i - 1) + (size_t)v.ie * ((size_t)j + nyn * ((size_t)(k - 1) + (size_t)v.ke * q))];
                    worst = std::max(worst, fabs(h - s[q])); scale = std::max(scale, fabs(h));
                }
                // sK(i, j, k), i = 1..ie, j = 1..je, k = 0..ke: v1 = x(i,j,k) - x(l,m,k) ; v2 = x(l,j,k) - x(i,m,k)
                node(i, j, k, n11); node(i - 1, j - 1, k, n10); node(i - 1, j, k, n01); node(i, j - 1, k, n00);
                cross(n11, n10, n01, n00, s);
                for (int q = 0; q < 3; ++q) {
                    const double h = d.sK[(size_t)(i - 1) + (size_t)v.ie * ((size_t)(j - 1) + (size_t)v.je * ((size_t)k + nzn * q))];
                    worst = std::max(worst, fabs(h - s[q])); scale = std::max(scale, fabs(h));
                }
            }
    return worst <= 1.e-11 * std::max(scale, 1.e-300);
}

int adflow_gpu_upload_geometry(int nn, int level, int sps)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    const adflow_block_desc& d = b->d;
    BlkView& v = b->v;
    // the marching kernels re-form face normals from the node coordinates and the viscous kernel derives its face vectors from
    // them: x is as much part of the geometry as the normals and the volumes
    if (!d.x || !d.sI || !d.sJ || !d.sK || !d.vol)
        return fail("block (%d,%d,%d): x, sI, sJ, sK and vol host arrays are required", nn, level, sps);
    int rc = 0;
    rc |= copy_box(b, v.x, d.x, 3, 0, v.ie + 1, 0, v.je + 1, 0, v.ke + 1, true);
    rc |= copy_box(b, v.sI, d.sI, 3, 0, v.ie + 1, 1, v.je, 1, v.ke, true);
    rc |= copy_box(b, v.sJ, d.sJ, 3, 1, v.ie, 0, v.je + 1, 1, v.ke, true);
    rc |= copy_box(b, v.sK, d.sK, 3, 1, v.ie, 1, v.je, 0, v.ke + 1, true);
    if (v.sFace) {
        rc |= copy_box(b, v.sFace, d.sFaceI, 1, 0, v.ie + 1, 1, v.je, 1, v.ke, true);
        rc |= copy_box(b, v.sFace + v.nbox, d.sFaceJ, 1, 1, v.ie, 0, v.je + 1, 1, v.ke, true);
        rc |= copy_box(b, v.sFace + 2 * v.nbox, d.sFaceK, 1, 1, v.ie, 1, v.je, 0, v.ke + 1, true);
    }
    rc |= copy_box(b, v.vol, d.vol, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    rc |= copy_box(b, v.volRef, d.volRef ? d.volRef : d.vol, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    rc |= copy_box(b, v.d2wall, d.d2Wall, 1, 2, v.nx, 2, v.ny, 2, v.nz, true);
    if (rc) return rc;
    // pack porosities + iblank into one byte per cell (internal.h)
    std::vector<uint8_t> f((size_t)v.nbox, 0);
    auto at = [&](int i, int j, int k) -> uint8_t& { return f[(size_t)v.idx(i, j, k)]; };
    if (d.porI)
        for (int k = 2; k <= v.kl; ++k)
            for (int j = 2; j <= v.jl; ++j)
                for (int i = 1; i <= v.il; ++i)
                    at(i, j, k) |= (uint8_t)((d.porI[(size_t)(i - 1) + (size_t)v.il * ((j - 2) + (size_t)v.ny * (k - 2))] + 1) & 3);
    if (d.porJ)
        for (int k = 2; k <= v.kl; ++k)
            for (int j = 1; j <= v.jl; ++j)
                for (int i = 2; i <= v.il; ++i)
                    at(i, j, k) |= (uint8_t)(((d.porJ[(size_t)(i - 2) + (size_t)v.nx * ((j - 1) + (size_t)v.jl * (k - 2))] + 1) & 3) << 2);
    if (d.porK)
        for (int k = 1; k <= v.kl; ++k)
            for (int j = 2; j <= v.jl; ++j)
                for (int i = 2; i <= v.il; ++i)
                    at(i, j, k) |= (uint8_t)(((d.porK[(size_t)(i - 2) + (size_t)v.nx * ((j - 2) + (size_t)v.ny * (k - 1))] + 1) & 3) << 4);
    for (int k = 0; k <= v.kb; ++k)
        for (int j = 0; j <= v.jb; ++j)
            for (int i = 0; i <= v.ib; ++i) {
                int ibl = d.iblank ? d.iblank[(size_t)i + (size_t)(v.ib + 1) * (j + (size_t)(v.jb + 1) * k)] : 1;
                if (ibl > 0) at(i, j, k) |= 64;
            }
    HIPCHK(hipMemcpyAsync(v.flags, f.data(), (size_t)b->boxsize, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    b->geom_uploaded = true;
    b->face_vectors_valid = false;
    b->geom_is_host = 15;
    b->normals_from_x_ok = normals_match_nodes(b);
    return 0;
}

// x only; adflow_gpu_update_geometry derives the rest on the device
int adflow_gpu_upload_coordinates(int nn, int level, int sps)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (!b->d.x) return fail("block (%d,%d,%d): no coordinate array", nn, level, sps);
    if (copy_box(b, b->v.x, b->d.x, 3, 0, b->v.ie + 1, 0, b->v.je + 1, 0, b->v.ke + 1, true)) return 1;
    b->face_vectors_valid = false;
    b->geom_is_host |= 1;
    // the stored sI / sJ / sK are now those of the OLD nodes: until update_geometry (or an upload of the new normals) re-forms
    // them no kernel may take its normals from x while another reads the arrays (two geometries in one residual)
    b->normals_from_x_ok = false;
    return sync_and_check();
}

// volume_block + metric_block + boundaryNormals (adjointExtra.F90:5-364) for every block of the level:
// the `useSpatial` branch of blocketteRes (blockette.F90:203-211) after the mesh moved
int adflow_gpu_update_geometry(int level)
{
    if (need_ready()) return 1;
    int rc = for_level(level, [&](Block* b) {
        if (!b->geom_uploaded) return fail("geometry of a level-%d block has not been uploaded", level);
        launch_volume_metric(b->v, b->d.rightHanded, g_stream);
        if (!b->bc.empty()) launch_boundary_normals(b->v, b->bc.data(), (int)b->bc.size(), g_stream);
        b->face_vectors_valid = false;
        b->geom_is_host &= 1;               // sI / sJ / sK were re-formed on the device: they are no longer the host arrays ...
        b->normals_from_x_ok = true;        // ... but they ARE metric_block(x) of the device's nodes
        return 0;
    });
    if (rc) return rc;
    return sync_and_check();
}

// flowDoms(nn,level,sps)%surfNodeIndices / %uv of determineWallAssociation (wallDistance.F90:1663-2002), kept on the device
int adflow_gpu_wall_distance_register(int nn, int level, int sps, const int32_t* surfNodeIndices, const double* uv)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (!surfNodeIndices || !uv) return fail("wall_distance_register: surfNodeIndices / uv is NULL");
    const size_t n = (size_t)b->v.nx * b->v.ny * b->v.nz;
    // largest surface node any cell refers to: update_wall_distances checks it against the xSurf it is handed
    int32_t mx = 0;
    for (size_t q = 0; q < 4 * n; ++q) {
        if (surfNodeIndices[q] < 0) return fail("wall_distance_register: negative surface node index");
        mx = std::max(mx, surfNodeIndices[q]);
    }
    b->wd_max_node = mx;
    if (!b->wd_ind) {
        void *pi = nullptr, *pu = nullptr;
        HIPCHK(hipMalloc(&pi, n * 4 * sizeof(int32_t)));
        b->allocs.push_back(pi);
        HIPCHK(hipMalloc(&pu, n * 2 * sizeof(double)));
        b->allocs.push_back(pu);
        b->wd_ind = (int*)pi;
        b->wd_uv = (double*)pu;
    }
    HIPCHK(hipMemcpyAsync(b->wd_ind, surfNodeIndices, n * 4 * sizeof(int32_t), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(b->wd_uv, uv, n * 2 * sizeof(double), hipMemcpyHostToDevice, g_stream));
    // the caller's arrays: consumed when the entry returns, whatever adflow_gpu_set_async says (from page-locked memory the copies
    // are truly asynchronous)
    HIPCHK(hipStreamSynchronize(g_stream));
    return sync_and_check();
}

static double* g_xsurf = nullptr;
static size_t g_xsurf_n = 0;

static void free_xsurf(void)
{
    if (g_xsurf) (void)hipFree(g_xsurf);
    g_xsurf = nullptr;
    g_xsurf_n = 0;
}

// updateWallDistancesQuickly (wallDistance.F90:36-120) for every block of the level with a registered association
int adflow_gpu_update_wall_distances(int level, const double* xSurf, int64_t n)
{
    if (need_ready()) return 1;
    if (n < 0 || (n > 0 && !xSurf) || n % 3) return fail("update_wall_distances: xSurf with %lld entries", (long long)n);
    if ((size_t)n > g_xsurf_n) {
        if (g_xsurf) (void)hipFree(g_xsurf);
        g_xsurf = nullptr; g_xsurf_n = 0;
        HIPCHK(hipMalloc((void**)&g_xsurf, sizeof(double) * (size_t)n));
        g_xsurf_n = (size_t)n;
    }
    if (n > 0) {
        // the caller refills xSurf after every warp: it is consumed before the entry returns, whatever adflow_gpu_set_async says;
        // the kernels behind the copy are only enqueued
        HIPCHK(hipMemcpyAsync(g_xsurf, xSurf, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    bool any = false;
    int rc = for_level(level, [&](Block* b) {
        if (!b->wd_ind) return 0;
        if (!b->geom_uploaded) return fail("geometry of a level-%d block has not been uploaded", level);
        if ((int64_t)3 * b->wd_max_node > n)
            return fail("update_wall_distances: the association of a level-%d block refers to surface node %d but xSurf holds %lld nodes",
                        level, b->wd_max_node, (long long)(n / 3));
        any = true;
        launch_wall_distance(b->v, b->wd_ind, b->wd_uv, g_xsurf, g_stream);
        return 0;
    });
    if (rc) return rc;
    (void)any;          // no association on this level (a level without walls): nothing to update, as updateWallDistancesQuickly
    return sync_and_check();
}

int adflow_gpu_upload_state(int nn, int level, int sps)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    const adflow_block_desc& d = b->d;
    BlkView& v = b->v;
    if (!d.w || !d.p || (!d.gamma && level == 1))
        return fail("block (%d,%d,%d): w, p and (on the finest level) gamma host arrays are required", nn, level, sps);
    int rc = 0;
    if (!d.gamma) {
        // coarse levels of the reference alias the fine level's gamma with fine strides (not handed over): constant gamma
        std::vector<double> g((size_t)(v.ib + 1) * (v.jb + 1) * (v.kb + 1), g_opts.gammaConstant);
        rc |= copy_box(b, v.gamma, g.data(), 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    }
    rc |= copy_box(b, v.w, d.w, v.nw, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    rc |= copy_box(b, v.p, d.p, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    rc |= copy_box(b, v.gamma, d.gamma, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    rc |= copy_box(b, v.rlv, d.rlv, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    rc |= copy_box(b, v.rev, d.rev, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, true);
    if (rc) return rc;
    b->ss_valid = false;
    b->etot_consistent = false;
    return sync_and_check();
}

int adflow_gpu_download_state(int nn, int level, int sps)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    const adflow_block_desc& d = b->d;
    BlkView& v = b->v;
    int rc = 0;
    rc |= copy_box(b, v.w, d.w, v.nw, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, false);
    rc |= copy_box(b, v.p, d.p, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, false);
    rc |= copy_box(b, v.rlv, d.rlv, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, false);
    rc |= copy_box(b, v.rev, d.rev, 1, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, false);
    if (rc) return rc;
    return sync_and_check();
}

int adflow_gpu_download_residual(int nn, int level, int sps)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (!b->d.dw) return fail("block (%d,%d,%d): no host dw array registered", nn, level, sps);
    BlkView& v = b->v;
    int rc = copy_box(b, v.dw, b->d.dw, v.nw, 0, v.ib + 1, 0, v.jb + 1, 0, v.kb + 1, false);
    if (rc) return rc;
    return sync_and_check();
}

static int array_spec(Block* b, int which, double** dev, int* nc, int lo[3], int n[3])
{
    BlkView& v = b->v;
    auto cell = [&]() { lo[0] = lo[1] = lo[2] = 0; n[0] = v.ib + 1; n[1] = v.jb + 1; n[2] = v.kb + 1; };
    auto halo1 = [&]() { lo[0] = lo[1] = lo[2] = 1; n[0] = v.ie; n[1] = v.je; n[2] = v.ke; };
    auto owned = [&]() { lo[0] = lo[1] = lo[2] = 2; n[0] = v.nx; n[1] = v.ny; n[2] = v.nz; };
    *nc = 1;
    switch (which) {
    case ADFLOW_ARR_W: *dev = v.w; *nc = v.nw; cell(); break;
    case ADFLOW_ARR_P: *dev = v.p; cell(); break;
    case ADFLOW_ARR_GAMMA: *dev = v.gamma; cell(); break;
    case ADFLOW_ARR_RLV: *dev = v.rlv; cell(); break;
    case ADFLOW_ARR_REV: *dev = v.rev; cell(); break;
    case ADFLOW_ARR_DW: *dev = v.dw; *nc = v.nw; cell(); break;
    case ADFLOW_ARR_FW: *dev = v.fw; *nc = 5; cell(); break;
    case ADFLOW_ARR_AA: *dev = v.aa; cell(); break;
    case ADFLOW_ARR_VOL: *dev = v.vol; cell(); break;
    case ADFLOW_ARR_DTL: *dev = v.dtl; halo1(); break;
    case ADFLOW_ARR_RADI: *dev = v.radI; halo1(); break;
    case ADFLOW_ARR_RADJ: *dev = v.radJ; halo1(); break;
    case ADFLOW_ARR_RADK: *dev = v.radK; halo1(); break;
    case ADFLOW_ARR_P1: *dev = v.p1; halo1(); break;
    case ADFLOW_ARR_W1: *dev = v.w1; *nc = 5; halo1(); break;
    case ADFLOW_ARR_WN: *dev = v.wn; *nc = 5; owned(); break;
    case ADFLOW_ARR_PN: *dev = v.pn; owned(); break;
    case ADFLOW_ARR_WR: *dev = v.wr; *nc = 5; owned(); break;
    case ADFLOW_ARR_NODAL_GRADS:
        *dev = v.grad; *nc = 12; lo[0] = lo[1] = lo[2] = 1; n[0] = v.il; n[1] = v.jl; n[2] = v.kl; break;
    case ADFLOW_ARR_D2WALL: *dev = v.d2wall; owned(); break;
    case ADFLOW_ARR_X: *dev = v.x; *nc = 3; lo[0] = lo[1] = lo[2] = 0; n[0] = v.ie + 1; n[1] = v.je + 1; n[2] = v.ke + 1; break;
    case ADFLOW_ARR_SI: *dev = v.sI; *nc = 3; lo[0] = 0; lo[1] = lo[2] = 1; n[0] = v.ie + 1; n[1] = v.je; n[2] = v.ke; break;
    case ADFLOW_ARR_SJ: *dev = v.sJ; *nc = 3; lo[1] = 0; lo[0] = lo[2] = 1; n[0] = v.ie; n[1] = v.je + 1; n[2] = v.ke; break;
    case ADFLOW_ARR_SK: *dev = v.sK; *nc = 3; lo[2] = 0; lo[0] = lo[1] = 1; n[0] = v.ie; n[1] = v.je; n[2] = v.ke + 1; break;
    default: return fail("unknown array id %d", which);
    }
    return 0;
}

int adflow_gpu_download_array(int nn, int level, int sps, int which, double* host)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (!host) return fail("null host pointer");
    double* dev; int nc, lo[3], n[3];
    if (array_spec(b, which, &dev, &nc, lo, n)) return 1;
    if (copy_box(b, dev, host, nc, lo[0], n[0], lo[1], n[1], lo[2], n[2], false)) return 1;
    return sync_and_check();
}

int adflow_gpu_upload_array(int nn, int level, int sps, int which, const double* host)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (!host) return fail("null host pointer");
    double* dev; int nc, lo[3], n[3];
    if (array_spec(b, which, &dev, &nc, lo, n)) return 1;
    if (copy_box(b, dev, host, nc, lo[0], n[0], lo[1], n[1], lo[2], n[2], true)) return 1;
    if (which == ADFLOW_ARR_W || which == ADFLOW_ARR_P || which == ADFLOW_ARR_GAMMA) {
        b->ss_valid = false;
        b->etot_consistent = false;
    }
    if (which == ADFLOW_ARR_X || which == ADFLOW_ARR_SI || which == ADFLOW_ARR_SJ || which == ADFLOW_ARR_SK) {
        // nodes or normals replaced one array at a time: the derived face vectors are stale.  The normals count as metric_block(x)
        // again only when the array came from the registered descriptor pointer (then the host arrays the check reads ARE what the
        // device holds); after an upload from any other buffer the stored normals are used until update_geometry / upload_geometry
        // (round-3 advisor finding)
        if (sync_and_check()) return 1;
        b->face_vectors_valid = false;
        const double* own = which == ADFLOW_ARR_X ? b->d.x : which == ADFLOW_ARR_SI ? b->d.sI : which == ADFLOW_ARR_SJ ? b->d.sJ : b->d.sK;
        const unsigned bit = which == ADFLOW_ARR_X ? 1u : which == ADFLOW_ARR_SI ? 2u : which == ADFLOW_ARR_SJ ? 4u : 8u;
        if (host == own) b->geom_is_host |= bit; else b->geom_is_host &= ~bit;
        // the host-side comparison speaks for the device only when ALL FOUR device arrays are the descriptor's: a foreign sI followed by
        // an upload of x from the registered pointer must not switch the re-formed normals back on
        b->normals_from_x_ok = b->geom_is_host == 15 && normals_match_nodes(b);
    }
    return sync_and_check();
}

// ---------------------------------------------------------------- hot path
int adflow_gpu_time_step(int level, int onlyRadii)
{
    if (need_ready()) return 1;
    KParams kp = make_kparams(level, 1.0, 0);
    kp.onlyRadii = onlyRadii;
    if (time_step_level(level, kp)) return 1;
    return sync_and_check();
}

int adflow_gpu_initres(int level, int varStart, int varEnd)
{
    if (need_ready()) return 1;
    if (varEnd < varStart) return 0;
    KParams kp = make_kparams(level, 1.0, 0);
    int rc = for_level(level, [&](Block* b) {
        if (varStart < 1 || varEnd > b->v.nw) return fail("initres: variable range %d..%d outside 1..%d", varStart, varEnd, b->v.nw);
        return 0;
    });
    if (rc) return rc;
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_initres_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, varStart - 1, varEnd - 1, g_stream);
    return sync_and_check();
}

// what this section calls of the sections further down (actuator sources, boundary conditions, wall stress, halo exchange)
static int source_terms_enqueue(int withBlank);
static int wall_stress_enqueue(int level, const KParams& kp, bool formGrad);
static bool has_wall_subfaces(int level);
static int apply_bc_enqueue(int level, int secondHalo);
static int apply_turb_and_flow_bc_enqueue(int level, int secondHalo, bool turbBC);
static int ad_apply_bc_enqueue(int level, const KParams& kp, bool turbBC);
static int halo_exchange_enqueue(int level, int varStart, int varEnd, int commPressure, int commVisc, int nLayers);
static int halo_exchange_close(int level, int varStart, int varEnd, int commPressure, int nLayers);
static int comm_exchange_begin(CommPattern* cp, BlkView* tab, unsigned mask, int nvar, bool* remoteOut);
static int comm_exchange_end(CommPattern* cp, BlkView* tab, unsigned mask, bool remote);

// blocks at rest: no grid velocities, no rotational source (only the generic kernels carry them)
static bool level_at_rest(int level)
{
    bool anyMoving = false;
    for_level(level, [&](Block* b) { anyMoving = anyMoving || b->v.sFace || b->v.moving; return 0; });
    return !anyMoving;
}

// dI / dJ / dK (and the cell centres) derived from x, once per geometry
static void block_face_vectors(Block* b)
{
    if (b->face_vectors_valid) return;
    launch_face_vectors(b->v, g_stream);
    b->face_vectors_valid = true;
}
static int ensure_face_vectors(int level)
{
    return for_level(level, [&](Block* b) { block_face_vectors(b); return 0; });
}

// the KParams of the evaluation block_res_enqueue(level, flags) runs (the Jacobian assembly plans with the same).  The forward-mode
// evaluation takes them too: its flags come from adflow_gpu_fd_jacobian alone, which never sets UPDATE_INTERMED (onlyRadii = 1) nor
// UPWIND_FIRST_ORDER, and g_rvec_target is set only while nk_residual_dev runs (no rvec)
static KParams res_kparams(int level, unsigned flags)
{
    KParams kp = make_kparams(level, 1.0, 0);
    kp.onlyRadii = !(flags & ADFLOW_RES_UPDATE_INTERMED);
    kp.coarseInit = 0;
    if (level == 1 && g_rvec_target) { kp.rvec = g_rvec_target; kp.rvecTurbScale = g_opts.turbResScale; }
    kp.dissApprox = (flags & ADFLOW_RES_DISS_APPROX) ? 1 : 0;
    if (kp.dissApprox && (flags & ADFLOW_RES_UPWIND_FIRST_ORDER)) kp.lumpedDiss = 1;   // blockette.F90:643
    kp.approxSA = (flags & ADFLOW_RES_APPROX_SA) ? 1 : 0;
    return kp;
}

// what plan_flow (flow_plan.h) reads, gathered in one place; resFlags: which parts the evaluation forms (ADFLOW_RES_FLOW / _TURB)
static FlowFacts flow_facts(int level, const KParams& kp, bool viscApprox, bool needGradHbm, bool dual = false,
                            unsigned resFlags = ADFLOW_RES_FLOW)
{
    FlowFacts f = {};
    f.spaceDiscr = kp.spaceDiscr; f.viscous = kp.viscous; f.fineGrid = kp.fineGrid; f.fwMode = kp.fwMode; f.dissApprox = kp.dissApprox;
    f.lumpedDiss = kp.lumpedDiss; f.limiter = kp.limiter; f.coarseInit = kp.coarseInit; f.onlyRadii = kp.onlyRadii;
    f.doScaling = kp.doScaling; f.rvec = kp.rvec != nullptr; f.rFil = kp.rFil; f.adis = kp.adis;
    f.viscApprox = viscApprox; f.needGradHbm = needGradHbm; f.dual = dual;
    f.wantFlow = (resFlags & ADFLOW_RES_FLOW) != 0; f.wantTurb = (resFlags & ADFLOW_RES_TURB) != 0;
    f.atRest = level_at_rest(level);
    f.rans = g_opts.equations == ADFLOW_RANS;
    f.eulerMarch = g_use_march; f.inviscidMarch = g_inviscid_march; f.roeMarch = g_roe_march; f.viscousTiled = g_viscous_tiled;
    f.saMarch = g_sa_march; f.pcFused = g_pc_fused; f.rvecJoint = g_rvec_joint; f.jacSnap = g_jac_snap;
    return f;
}

// ---- forward-mode linearisation (kernels_ad.hip): dual copies of the arrays the kernels touch, laid out by ad_prepare below ---------
struct AdInit { char* dst; const double* src; size_t n, zeroBytes; };   // dual array at dst: (src, 0) for n entries, or zeroBytes of zero
struct AdBlock { BlkView v; std::vector<AdInit> init; };
static std::map<Block*, AdBlock> g_ad;
static BlkView* g_ad_tab = nullptr;        // device table of the level being linearised, slot layout of g_tab[level]

// The two families of launchers of one evaluation in one shape: PLAIN on the library's arrays, DUAL on the dual copies of the forward
// mode.  The executors below launch what a FlowPlan names through one of them.  What else differs between the modes hangs on `dual`
// and is said where it happens: only PLAIN records phase marks, checks geom_uploaded, refreshes the entropy sensor, keeps the
// ss_valid / etot_consistent bookkeeping of the arrays it writes and calls the host hook.
struct Launchers {
    using Tiles = void (*)(const BlkView*, const int4*, int, const KParams&, hipStream_t);
    using TilesRc = int (*)(const BlkView*, const int4*, int, const KParams&, hipStream_t);
    using Level = void (*)(const BlkView*, int, int, int, int, const KParams&, hipStream_t);
    using OneBlock = void (*)(const BlkView&, const KParams&, hipStream_t);
    bool dual;
    const BlkView& (*view)(Block* b);                                   // the arrays of one block (the level's table: mode_tab)
    OneBlock closures_halo;
    int (*bcs)(int level, const KParams& kp, bool turbBC);              // turbulence + mean-flow boundary conditions, both halos
    Tiles sa_march;
    Level sa_residual_level;
    Tiles euler_march;                                                  // (no dual form)
    TilesRc roe_march, inviscid_march;
    void (*pc_march)(const BlkView*, const int4*, int, const KParams&, int kch, hipStream_t);
    Level inviscid_level;
    void (*visc_gf)(const BlkView*, const int4*, int, const KParams&, bool storeGrad, hipStream_t);
    Tiles visc_march_approx;
    OneBlock viscous, viscous_approx;
};
static const Launchers PLAIN = {
    false,
    [](Block* b) -> const BlkView& { return b->v; },
    launch_closures_halo,
    [](int level, const KParams&, bool turbBC) { return apply_turb_and_flow_bc_enqueue(level, 1, turbBC); },
    [](const BlkView* tab, const int4* tiles, int n, const KParams& kp, hipStream_t s) { launch_sa_march(tab, tiles, n, kp, s, false); },
    launch_sa_residual_level,
    launch_euler_march,
    launch_roe_march, launch_inviscid_march,
    launch_pc_march,
    launch_inviscid_level,
    launch_visc_gf,
    launch_visc_march_approx,
    launch_viscous, launch_viscous_approx};
static const Launchers DUAL = {
    true,
    [](Block* b) -> const BlkView& { return g_ad[b].v; },
    ad_launch_closures_halo,
    ad_apply_bc_enqueue,
    ad_launch_sa_march,
    ad_launch_sa_residual_level,
    nullptr,
    ad_launch_roe_march, ad_launch_inviscid_march,
    ad_launch_pc_march,
    ad_launch_inviscid_level,
    [](const BlkView* tab, const int4* tiles, int n, const KParams& kp, bool, hipStream_t s) { ad_launch_visc_gf(tab, tiles, n, kp, s); },
    ad_launch_visc_march_approx,
    ad_launch_viscous, ad_launch_viscous_approx};

// block table and launch extents of the level in the arrays of the mode
static int mode_tab(const Launchers& M, int level, LevelTab* t)
{
    if (level_tab(level, t)) return 1;
    if (M.dual) t->tab = g_ad_tab;
    return 0;
}

// the turbulence kernel the plan names
static int enqueue_turb_residual(const Launchers& M, int level, const FlowPlan& P, const KParams& kp)
{
    if (P.turb == TurbK::None) return 0;
    int rc = for_level(level, [&](Block* b) {
        if (b->v.nw < 6) return fail("RANS/SA needs nw = 6 (block has %d)", b->v.nw);
        return 0;
    });
    if (rc) return rc;
    LevelTab t;
    if (mode_tab(M, level, &t)) return 1;
    if (P.turb == TurbK::SaMarch) {
        if (ensure_sa_tiles(level)) return 1;
        M.sa_march(t.tab, g_sa_tiles[level].first, g_sa_tiles[level].second, kp, g_stream);
    } else M.sa_residual_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, g_stream);
    return 0;
}

// one mean-flow kernel of the plan; the tile tables it reads exist (FlowPlan::needTiles / needGfTiles, ensured by the caller)
static int enqueue_inviscid(const Launchers& M, int level, InviscidK which, const KParams& kv)
{
    LevelTab t;
    if (mode_tab(M, level, &t)) return 1;
    switch (which) {
    case InviscidK::EulerMarch:
        if (!M.euler_march) break;
        M.euler_march(t.tab, g_tiles[level].first, g_tiles[level].second, kv, g_stream);
        return 0;
    case InviscidK::RoeMarch: return M.roe_march(t.tab, g_tiles[level].first, g_tiles[level].second, kv, g_stream);
    case InviscidK::FaceMarch: return M.inviscid_march(t.tab, g_tiles[level].first, g_tiles[level].second, kv, g_stream);
    case InviscidK::PcMarch: M.pc_march(t.tab, g_tiles[level].first, g_tiles[level].second, kv, g_march_kch, g_stream); return 0;
    case InviscidK::LevelGather: M.inviscid_level(t.tab, t.n, t.nx, t.ny, t.nz, kv, g_stream); return 0;
    case InviscidK::None: return 0;
    }
    return fail("forward mode: the plan names a kernel without a dual form (internal error)");
}
static int enqueue_viscous(const Launchers& M, int level, ViscousK which, const KParams& kv, bool storeGrad)
{
    LevelTab t;
    if (mode_tab(M, level, &t)) return 1;
    // (DUAL: ad_prepare formed the face vectors of a viscous level already, block_face_vectors launches nothing)
    auto per_block = [&](Launchers::OneBlock launch) {
        return for_level(level, [&](Block* b) { block_face_vectors(b); launch(M.view(b), kv, g_stream); return 0; });
    };
    switch (which) {
    case ViscousK::GfMarch: M.visc_gf(t.tab, g_gf_tiles[level].first, g_gf_tiles[level].second, kv, storeGrad, g_stream); return 0;
    case ViscousK::ThinLayerMarch: M.visc_march_approx(t.tab, g_tiles[level].first, g_tiles[level].second, kv, g_stream); return 0;
    case ViscousK::GatherExact: return per_block(M.viscous);
    case ViscousK::GatherApprox: return per_block(M.viscous_approx);
    case ViscousK::None: break;
    }
    return 0;
}

// the mean-flow fluxes the plan names, in its order (phase marks, PLAIN only: 4 .. 5 = nodal gradients + viscous fluxes, 5 .. 6 =
// inviscid fluxes when they follow; bench.py labels them so).  On dual numbers these are the marching kernels compiled a second time
// (kernels_ad.hip) -- the Roe march of the exact linearisation (3.25 instead of 6 face evaluations and 3.5 instead of 12
// reconstructions per cell), the per-face march of scalar JST / matrix dissipation (four face evaluations per cell instead of the
// gather kernel's six), the one-march residual of the preconditioner matrix, k_visc_gf (instead of the dual gather pair
// k_nodal_gradients + k_viscous: 1.01 ms per pass and 1.3 M cells) -- or the gather kernels behind them
static int enqueue_flow_fluxes(const Launchers& M, int level, const KParams& kp, const FlowPlan& P, bool needGrad)
{
    if (!M.dual) {
        if (kp.spaceDiscr != ADFLOW_DISS_SCALAR && kp.spaceDiscr != ADFLOW_DISS_MATRIX && kp.spaceDiscr != ADFLOW_UPWIND)
            return fail("spaceDiscr=%d not supported (1 scalar, 2 matrix, 9 upwind)", kp.spaceDiscr);
        int nStale = 0, nBlk = 0;
        int rc = for_level(level, [&](Block* b) {
            if (!b->geom_uploaded) return fail("geometry of a level-%d block has not been uploaded", level);
            ++nBlk;
            if (P.needSensor && !b->ss_valid) ++nStale;
            return 0;
        });
        if (rc) return rc;
        if (nStale > 0) {
            // entropy sensor of the blocks whose state changed: one launch when that is every block of the level (the usual case)
            if (nStale == nBlk) {
                LevelTab ts;
                if (level_tab(level, &ts)) return 1;
                launch_entropy_level(ts.tab, ts.n, ts.nx, ts.ny, ts.nz, g_stream);
            }
            for_level(level, [&](Block* b) {
                if (nStale != nBlk && !b->ss_valid) launch_entropy(b->v, g_stream);
                b->ss_valid = true;
                return 0;
            });
        }
    }
    // dI / dJ / dK: DUAL forms them before any flux kernel, PLAIN in front of the viscous kernel
    if (M.dual && P.needFaceVectors && ensure_face_vectors(level)) return 1;
    if ((P.needGfTiles && ensure_gf_tiles(level)) || (P.needTiles && ensure_tiles(level))) return 1;
    KParams kv = kp;
    kv.viscFirst = P.viscFirst ? 1 : 0;
    auto mark = [&](int i) { if (!M.dual) phase_mark(i); };
    auto inviscid = [&]() { return enqueue_inviscid(M, level, P.inviscid, kv); };
    auto viscous = [&]() { return enqueue_viscous(M, level, P.viscous, kv, needGrad); };
    if (P.inviscid == InviscidK::EulerMarch) return inviscid();          // (no viscous part, one phase)
    const bool pc = P.inviscid == InviscidK::PcMarch;                     // (it carries the viscous part: between the marks 4 and 5)
    if (pc || P.viscFirst) {
        if (!M.dual && ensure_face_vectors(level)) return 1;
        mark(4);
        if (pc ? inviscid() : viscous()) return 1;
        mark(5);
        return pc ? 0 : inviscid();
    }
    if (inviscid()) return 1;
    mark(4);
    if (!M.dual && P.needFaceVectors && ensure_face_vectors(level)) return 1;
    if (P.viscous == ViscousK::GfMarch) mark(5);
    return viscous();
}

// residual (residuals.F90:1028) = residual_block of every block; blockResCore (blockette.F90:755) is the same sum of
// fluxes WITHOUT the low-speed preconditioner of residual_block (residuals.F90:172-331) -> lowSpeed = false there.
// stage0: the reference's rkStage is 0 at this call -> on the ground level viscousFlux also stores the wall stress tensor
// and heat flux of the viscous subfaces (storeWallTensor, fluxes.F90:2586-2592)
// needGradHbm: the caller wants the nodal gradients in the block arrays (updateIntermed copy-out, blockette.F90:706-750)
static int enqueue_flow_residual(int level, const KParams& kp, bool viscApprox = false, bool lowSpeed = true, bool stage0 = true,
                                 bool needGradHbm = false)
{
    const bool wallStress = stage0 && !viscApprox && kp.viscous && level == g_opts.groundLevel && fabs(kp.rFil) >= 1.e-10 &&
                            has_wall_subfaces(level);
    const FlowPlan P = plan_flow(flow_facts(level, kp, viscApprox, needGradHbm));
    if (enqueue_flow_fluxes(PLAIN, level, kp, P, needGradHbm)) return 1;
    if (wallStress)
        if (wall_stress_enqueue(level, kp, P.wallGradOnChip)) return 1;
    // sourceTerms() of the call sites of `residual` (smoothers.F90:74,409, multiGrid.F90:52,887,949): fine level only
    if (lowSpeed && level == 1 && source_terms_enqueue(1)) return 1;
    if (lowSpeed && g_opts.lowSpeedPreconditioner) {
        LevelTab t;
        if (level_tab(level, &t)) return 1;
        launch_low_speed_precond_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, g_stream);
    }
    return 0;
}

int adflow_gpu_residual(int level, int rkStage)
{
    if (need_ready()) return 1;
    double rFil = 1.0;
    int fwMode = 0;
    if (g_opts.smoother == ADFLOW_RUNGE_KUTTA) {
        if (rkStage < 0 || rkStage >= g_opts.nRKStages) return fail("rkStage=%d outside 0..%d", rkStage, g_opts.nRKStages - 1);
        rFil = g_opts.cdisRK[rkStage];   // cdisRK(rkStage+1), residuals.F90:61-65
        fwMode = 1;
    }
    KParams kp = make_kparams(level, rFil, fwMode);
    int rc = enqueue_flow_residual(level, kp, false, true, rkStage == 0);
    if (rc) return rc;
    return sync_and_check();
}

// whalo2 + blocketteRes core with the exchange -- and, round 4, the boundary conditions in front of it -- HIDDEN behind the tiles that
// read no halo cell (round-2 verdict, next 3 iii).  Two queues from the fork behind the derived values:
//   main queue:  boundary conditions (frontBCs), packs, RCCL group on the communication queue, same-GPU copies, wait for the group,
//                unpacks, periodic transforms, whalo2's closing energy; then the fused viscous march over the BOUNDARY tiles, the
//                inviscid march over every tile (it adds the viscous sums), the wall stress
//   side queue:  SA march and fused viscous march over their INTERIOR tiles (they read owned cells only: neither a boundary halo
//                nor an exchanged one) -- while the boundary kernels (a few hundred workgroups each) and the copies leave the chip
//                idle; then, behind the exchange, the SA march over the boundary tiles
// Taken for the default flags of blocketteRes on NS / RANS with the marching kernels, blocks at rest, when the pattern has messages
// (tuning "split_eval" = 1, the default), always (2: tests), never (0).  On the north-star mesh
// 16 % of the tiles are interior.
static int block_res_split_enqueue(int level, unsigned flags, const KParams& kp, const FlowPlan& P, int lStart, int lEnd, int* taken,
                                   const std::function<int()>& frontBCs)
{
    *taken = 0;
    if (!g_split_eval || !g_overlap || g_phase_base > 0 || kp.rvec) return 0;
    const unsigned need = ADFLOW_RES_FLOW | ADFLOW_RES_HALO;
    if ((flags & need) != need || (flags & (ADFLOW_RES_DISS_APPROX | ADFLOW_RES_VISC_APPROX | ADFLOW_RES_UPDATE_INTERMED))) return 0;
    // the evaluation the split is written for: fused viscous march in front of an inviscid march over the tile table, SA as a march, no
    // time-step pass in front (scalar JST: not split), fine level
    if (P.viscous != ViscousK::GfMarch || !P.viscFirst || (P.inviscid != InviscidK::RoeMarch && P.inviscid != InviscidK::FaceMarch) ||
        P.turb == TurbK::LevelGather || P.needTimeStep || !kp.fineGrid) return 0;
    const bool rans = P.turb == TurbK::SaMarch;
    const bool wall = has_wall_subfaces(level) && level == g_opts.groundLevel;
    if (!g_act.empty()) return 0;
    CommPattern* cp;
    if (build_comm(level, 2, &cp)) return 1;
    const bool messages = !cp->sends.empty() || !cp->recvs.empty();
    // (boundary subfaces alone do not make it pay: measured on the wall-bounded bench mesh at N = 1 the split costs 0.03 ms --
    //  2.45 against 2.42 ms -- the two extra launches per kernel outweigh what the interior tiles hide of the boundary kernels)
    if (g_split_eval < 2 && !messages) return 0;
    if (g_bc_callback) return 0;               // (a host hook between the device passes synchronises the queue)
    unsigned mask; int nvar;
    if (halo_mask(lStart, lEnd, 1, 1, &mask, &nvar)) return 1;
    if (nvar == 0) return 0;
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    int rc = for_level(level, [&](Block* b) {
        if (!b->geom_uploaded) return fail("geometry of a level-%d block has not been uploaded", level);
        if (rans && b->v.nw < 6) return fail("RANS/SA needs nw = 6 (block has %d)", b->v.nw);
        block_face_vectors(b);
        return 0;
    });
    if (rc) return rc;
    if (ensure_tiles(level) || ensure_gf_tiles(level) || (rans && ensure_sa_tiles(level))) return 1;
    *taken = 1;
    KParams kv = kp;
    kv.viscFirst = 1;
    // (everything behind the fork runs inside `run`: an error exit must not leave the side queue unjoined -- round-3 advisor finding)
    bool forked = false;
    auto run = [&]() -> int {
        // ---- fork behind the derived values: the halo-free tiles on the side queue
        HIPCHK(hipEventRecord(g_evFork, g_stream));
        HIPCHK(hipStreamWaitEvent(g_streamB, g_evFork, 0));
        forked = true;
        if (rans) launch_sa_march(t.tab, g_sa_tiles_int[level].first, g_sa_tiles_int[level].second, kp, g_streamB, false);
        launch_visc_gf(g_tab[level], g_gf_tiles_int[level].first, g_gf_tiles_int[level].second, kv, false, g_streamB);
        HIPCHK(hipEventRecord(g_evB1, g_streamB));
        // ---- main queue: boundary conditions, messages out, same-GPU copies, messages in
        if (frontBCs()) return 1;
        if (g_test_fault & 2) return fail("test_fault: the split evaluation fails behind its fork");
        bool remote = false;
        if (comm_exchange_begin(cp, g_tab[level], mask, nvar, &remote)) return 1;
        if (comm_exchange_end(cp, g_tab[level], mask, remote)) return 1;
        if (halo_exchange_close(level, lStart, lEnd, 1, 2)) return 1;
        // ---- the tiles next to the block faces, then the inviscid march over all of them
        HIPCHK(hipEventRecord(g_evC, g_stream));
        HIPCHK(hipStreamWaitEvent(g_streamB, g_evC, 0));
        if (rans) launch_sa_march(t.tab, g_sa_tiles_bnd[level].first, g_sa_tiles_bnd[level].second, kp, g_streamB, false);
        HIPCHK(hipEventRecord(g_evB, g_streamB));
        launch_visc_gf(g_tab[level], g_gf_tiles_bnd[level].first, g_gf_tiles_bnd[level].second, kv, false, g_stream);
        HIPCHK(hipStreamWaitEvent(g_stream, g_evB1, 0));               // the interior viscous sums are in dw(2:5)
        if (enqueue_inviscid(PLAIN, level, P.inviscid, kv)) return 1;
        HIPCHK(hipStreamWaitEvent(g_stream, g_evB, 0));                // join
        forked = false;
        return 0;
    };
    if (run()) {
        if (forked && hipEventRecord(g_evB, g_streamB) == hipSuccess) (void)hipStreamWaitEvent(g_stream, g_evB, 0);
        return 1;
    }
    // viscSubface%tau / %q (storeWall, blockette.F90:135): from the node planes on the wall faces, formed behind the exchange
    if (wall && wall_stress_enqueue(level, kp, true)) return 1;
    return 0;
}

namespace {
// ADFLOW_RES_TURB_FIRST_ORDER: orderTurb = firstOrder for one evaluation (NKSolvers.F90:3411-3412, :3855-3856), restored on every exit
struct OrderTurbGuard {
    const int was;
    explicit OrderTurbGuard(bool firstOrder) : was(g_opts.orderTurb) { if (firstOrder) g_opts.orderTurb = 1; }
    ~OrderTurbGuard() { g_opts.orderTurb = was; }
};
}  // namespace

static int block_res_enqueue(int level, unsigned flags)
{
    if (need_ready()) return 1;
    OrderTurbGuard orderGuard((flags & ADFLOW_RES_TURB_FIRST_ORDER) != 0);
    phase_mark(0);
    KParams kp = res_kparams(level, flags);
    const bool viscApprox = (flags & ADFLOW_RES_VISC_APPROX) != 0;
    const FlowPlan P = plan_flow(flow_facts(level, kp, viscApprox, (flags & ADFLOW_RES_UPDATE_INTERMED) != 0, false, flags));
    int rc = 0;
    bool etotInClosures = false;
    if (flags & ADFLOW_RES_CLOSURES) {
        // computePressureSimple / computeLamViscosity / computeEddyViscosity (blockette.F90:199-203)
        LevelTab tc;
        if (level_tab(level, &tc)) return 1;
        // when the whalo2 of this call follows (mean-flow variables incl. the energy), the energy it would recompute on the owned
        // cells is written by the same pass wherever the pressure kept its value (as FormFunction_mf does, kernels_nk.hip
        // closures_body): a floored cell raises the device flag and whalo2's closing pass runs only then.  (The reference sends the old
        // energy and recomputes afterwards, haloExchange.F90:154-196: a neighbour's halo energy differs by the rounding of p -> E -> p,
        // DESIGN 4 round 4 (c))
        etotInClosures = (flags & ADFLOW_RES_HALO) && (flags & ADFLOW_RES_FLOW) && g_comm.count(std::make_pair(level, 2)) > 0;
        if (etotInClosures) {
            if (!g_floor_flag_dev) HIPCHK(hipMalloc((void**)&g_floor_flag_dev, sizeof(int)));
            HIPCHK(hipMemsetAsync(g_floor_flag_dev, 0, sizeof(int), g_stream));
        }
        launch_closures_level(tc.tab, tc.n, tc.nx, tc.ny, tc.nz, kp, g_stream, etotInClosures ? g_floor_flag_dev : nullptr);
        rc = for_level(level, [&](Block* b) {
            b->ss_valid = false;
            b->etot_consistent = false;
            return 0;
        });
        if (rc) return rc;
    }
    if (flags & ADFLOW_RES_HALO) {
        // BCTurbTreatment + applyAllTurbBCThisBlock(.true.) before applyAllBC_block(.true.) (blockette.F90:220-226)
        auto frontBCs = [&]() -> int {
            if (apply_turb_and_flow_bc_enqueue(level, 1, (flags & ADFLOW_RES_TURB) != 0)) return 1;
            if (g_bc_callback) {
                HIPCHK(hipStreamSynchronize(g_stream));
                g_bc_callback(level, 1);
            }
            return 0;
        };
        int lStart = 1, lEnd = (g_opts.equations == ADFLOW_RANS) ? 6 : 5;
        if ((flags & ADFLOW_RES_FLOW) && !(flags & ADFLOW_RES_TURB)) lEnd = 5;
        if (!(flags & ADFLOW_RES_FLOW) && (flags & ADFLOW_RES_TURB)) lStart = 6;
        if (g_comm.count(std::make_pair(level, 2))) {
            // the boundary conditions and the exchange with the halo-free tiles of the evaluation beside them, where the evaluation
            // is the marching RANS / NS one
            int taken = 0;
            const int flagLevelWas = g_etot_flag_level;
            if (etotInClosures) g_etot_flag_level = level;
            rc = block_res_split_enqueue(level, flags, kp, P, lStart, lEnd, &taken, frontBCs);
            if (!rc && !taken) {
                rc = frontBCs();
                if (!rc) rc = halo_exchange_enqueue(level, lStart, lEnd, 1, 1, 2);
            }
            g_etot_flag_level = flagLevelWas;
            if (rc) return 1;
            if (taken) return 0;
        } else if (frontBCs()) return 1;
    }
    phase_mark(1);
    kp.radiiInMarch = P.radiiInMarch ? 1 : 0;
    if (P.needTimeStep) {
        rc = time_step_level(level, kp);
        if (rc) return rc;
    }
    phase_mark(2);
    if (P.roeWritesTurbRvec) kp.rvecTurbFromDw = 1;
    if (enqueue_turb_residual(PLAIN, level, P, kp)) return 1;
    phase_mark(3);
    if (flags & ADFLOW_RES_FLOW) {
        rc = enqueue_flow_residual(level, kp, viscApprox, false, true, (flags & ADFLOW_RES_UPDATE_INTERMED) != 0);
        if (rc) return rc;
    }
    phase_mark(6);
    // actuator-region sources after the core, fine level only and without the iblank factor (blockette.F90:276-281)
    if (level == 1 && source_terms_enqueue(0)) return 1;
    return 0;
}

// ---- actuator regions (actuatorRegionData.F90) -----------------------------------------------------------------------
int adflow_gpu_actuator_register(int nRegions, const adflow_actuator_region* regions)
{
    ++g_state_gen;
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    if (nRegions < 0 || (nRegions > 0 && !regions)) return fail("actuator_register: nRegions=%d", nRegions);
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    for (auto& r : g_act) free_list(r.list);
    g_act.clear();
    for (int m = 0; m < nRegions; ++m) {
        const adflow_actuator_region& in = regions[m];
        const int n = in.nCellIDs;
        if (n < 0 || (n > 0 && (!in.block || !in.cellIDs))) return fail("actuator_register: region %d: nCellIDs=%d", m + 1, n);
        if (!(in.volume > 0.0)) return fail("actuator_register: region %d: volume must be positive", m + 1);
        ActRegion r;
        r.h_block.assign(in.block, in.block + n);
        r.h_idx.resize((size_t)3 * n);
        for (int t = 0; t < n; ++t)
            for (int q = 0; q < 3; ++q) r.h_idx[(size_t)q * n + t] = in.cellIDs[(size_t)3 * t + q];   // (3,n) -> (n,3)
        for (int q = 0; q < 3; ++q) r.force[q] = in.force[q];
        r.heat = in.heat; r.volume = in.volume; r.relaxStart = in.relaxStart; r.relaxEnd = in.relaxEnd;
        g_act.push_back(r);
    }
    return 0;
}

static int source_terms_enqueue(int withBlank)
{
    if (g_act.empty()) return 0;
    if (ensure_table(1)) return 1;
    for (auto& r : g_act) {
        const int n = (int)r.h_block.size();
        if (!r.built) {
            free_list(r.list);
            r.list.n = n;
            if (n > 0 && make_list(1, r.h_block.data(), r.h_idx.data(), n, 0, n, &r.list.blkA, &r.list.offA)) return 1;
            r.built = true;
        }
        // relaxation factor and the non-dimensional scales (residuals.F90:367-385)
        double factor;
        const double oc = g_opts.ordersConverged;
        if (oc < r.relaxStart) factor = 0.0;
        else if (oc > r.relaxEnd) factor = 1.0;
        else factor = (oc - r.relaxStart) / (r.relaxEnd - r.relaxStart);
        double Ff[3];
        for (int q = 0; q < 3; ++q) Ff[q] = factor * r.force[q] / r.volume / g_opts.pRef;
        const double Qf = factor * r.heat / r.volume / (g_opts.pRef * g_opts.uRef * g_opts.LRef * g_opts.LRef);
        launch_source_terms(g_tab[1], r.list.blkA, r.list.offA, n, Ff, Qf, withBlank, g_stream);
    }
    return 0;
}

// referenceShockSensor (adjointUtils.F90:1909-1969): pressure (Euler or matrix dissipation) or entropy
static int reference_shock_sensor_enqueue(int level)
{
    const bool pressure = (g_opts.equations == ADFLOW_EULER) || (g_opts.spaceDiscr == ADFLOW_DISS_MATRIX);
    return for_level(level, [&](Block* b) {
        if (pressure) HIPCHK(hipMemcpyAsync(b->v.ss, b->v.p, sizeof(double) * (size_t)b->boxsize, hipMemcpyDeviceToDevice, g_stream));
        else launch_entropy(b->v, g_stream);
        return 0;
    });
}

int adflow_gpu_reference_shock_sensor(int level)
{
    if (need_ready()) return 1;
    if (reference_shock_sensor_enqueue(level)) return 1;
    // the exact viscous kernel recomputes its own sensor after an approximate pass
    for_level(level, [&](Block* b) { b->ss_valid = false; return 0; });
    return sync_and_check();
}

int adflow_gpu_block_res(int level, unsigned flags)
{
    int rc = block_res_enqueue(level, flags);
    if (rc) return rc;
    return sync_and_check();
}

// ---- coloured finite-difference Jacobian (adjointUtils::setupStateResidualMatrix, useAD = F; adjointUtils.F90:7-715) ----------
static JacSpec g_jac;                 // stencil / colouring / state range of the last assembly

static void jac_spec(unsigned flags, bool viscous, bool rans, JacSpec* J)
{
    memset(J, 0, sizeof *J);
    // state range (adjointUtils.F90:85-106)
    if (flags & ADFLOW_JAC_TURB_ONLY) { J->lStart = 5; J->nState = 1; }
    else { J->lStart = 0; J->nState = (rans && !(flags & ADFLOW_JAC_FROZEN_TURB)) ? 6 : 5; }
    int n = 0;
    auto add = [&](int a, int b, int c) { J->st[n][0] = a; J->st[n][1] = b; J->st[n][2] = c; ++n; };
    auto star = [&](int r) { add(-r, 0, 0); add(r, 0, 0); add(0, -r, 0); add(0, r, 0); add(0, 0, -r); add(0, 0, r); };
    if (flags & ADFLOW_JAC_PC) {
        add(0, 0, 0); star(1);                                          // euler_pc_stencil (stencils.f90:34-40)
        if (viscous && (flags & ADFLOW_JAC_VISC_PC)) {                  // visc_pc_stencil (:60-85), setup_3x3x3_coloring
            for (int c = -1; c <= 1; ++c)
                for (int b = -1; b <= 1; ++b)
                    for (int a = -1; a <= 1; ++a)
                        if ((a != 0) + (b != 0) + (c != 0) >= 2) add(a, b, c);
            J->ca = 1; J->cb = 3; J->cc = 9; J->cn = 27; J->cm = 3;
        } else {
            J->ca = 1; J->cb = 5; J->cc = 4; J->cn = 7; J->cm = 7;      // setup_PC_coloring (adjointUtils.F90:1089-1119)
        }
    } else if (viscous) {
        for (int c = -1; c <= 1; ++c)                                   // visc_drdw_stencil (stencils.f90:87-106)
            for (int b = -1; b <= 1; ++b)
                for (int a = -1; a <= 1; ++a) add(a, b, c);
        star(2);
        J->ca = 1; J->cb = 19; J->cc = 11; J->cn = 35; J->cm = 35;      // setup_dRdw_visc_coloring (:1153-1183)
    } else {
        add(0, 0, 0);                                                   // euler_drdw_stencil (stencils.f90:42-55)
        for (int d = 0; d < 3; ++d)
            for (int r : {-2, -1, 1, 2}) add(d == 0 ? r : 0, d == 1 ? r : 0, d == 2 ? r : 0);
        J->ca = 1; J->cb = 3; J->cc = 4; J->cn = 13; J->cm = 13;        // setup_dRdw_euler_coloring (:1121-1151)
    }
    J->nStencil = n;
    for (int q = 0; q < n; ++q) {
        const int v = (J->ca * J->st[q][0] + J->cb * J->st[q][1] + J->cc * J->st[q][2]) % J->cn;
        J->sc[q] = (v < 0) ? v + J->cn : v;
    }
}

// viscPC: block_res_state_d keeps the FULL viscous flux in the preconditioner matrix then (masterRoutines.F90:1380: `.not. lumpedDiss
// .or. viscPC`) -- unlike the finite-difference path block_res_state, whose viscApprox = lumpedDiss whatever viscPC says (:1269-1270)
static bool visc_approx(const Launchers& M, unsigned resFlags, bool viscPC)
{
    return (resFlags & ADFLOW_RES_VISC_APPROX) != 0 && !(M.dual && viscPC);
}

// masterRoutines::block_res_state (masterRoutines.F90:1214-1283) for every block of the level, or block_res_state_d (:1285-1393) on
// its dual arrays: closures with halos, turbulence and mean-flow boundary conditions, host hook, the residual core -- PLAIN: that of
// block_res_enqueue with the actuator sources; DUAL: time step (the spectral radii of the scalar dissipation), SA, fluxes.  resScale
// is applied by the extraction kernel.
// closuresDone: the state / seed launch of the caller formed pressure and viscosities already
static int block_res_state_enqueue(const Launchers& M, int level, unsigned resFlags, bool turbBC, bool viscPC, bool closuresDone = false)
{
    const KParams kp = res_kparams(level, resFlags);
    int rc = for_level(level, [&](Block* b) {
        if (!closuresDone) M.closures_halo(M.view(b), kp, g_stream);
        if (!M.dual) {
            b->ss_valid = false;
            b->etot_consistent = false;
        }
        return 0;
    });
    if (rc) return rc;
    if (M.bcs(level, kp, turbBC)) return 1;
    // (the forward-mode assembly refuses host hooks before it starts)
    if (!M.dual && g_bc_callback) {
        HIPCHK(hipStreamSynchronize(g_stream));
        g_bc_callback(level, 1);
    }
    if (!M.dual) return block_res_enqueue(level, resFlags);
    const FlowPlan P = plan_flow(flow_facts(level, kp, visc_approx(M, resFlags, viscPC), false, true, resFlags));
    LevelTab t;
    if (mode_tab(M, level, &t)) return 1;
    // timeStep_block_d: the NS / RANS kernel also leaves the entropy sensor in ss -- not under dissApprox, where ss keeps the frozen
    // sensor of referenceShockSensor (value part, derivative 0)
    if (P.needTimeStep) ad_launch_time_step_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, g_stream);
    if (enqueue_turb_residual(M, level, P, kp)) return 1;
    return enqueue_flow_fluxes(M, level, kp, P, false);
}

// ---- forward-mode linearisation: the slab of the dual arrays ---------------------------------------------------------------------
// Round 5 (round-4 advisor): ONE slab per level instead of ~57 hipMalloc / hipFree per block and call, kept between calls (tuning
// "ad_cache", default 1; dropped when a block is released or the level's layout changes) -- on the north-star mesh the 13.5 GB (8.4 GB since the geometry is no longer copied) of
// dual arrays cost 0-400 ms per assembly to map, depending on the box (profiles/r05_f_bench.json against r05_d) -- and the free
// memory is checked before the slab is requested.
static char* g_ad_slab = nullptr;
static size_t g_ad_slab_bytes = 0, g_ad_bump = 0;
static bool g_ad_measure = false;
static std::vector<long> g_ad_sig;         // what the cached slab was laid out for
int g_ad_cache = 1;

static void ad_drop();
static void ad_cache_drop() { ad_drop(); }
static void ad_drop()
{
    g_ad.clear();
    if (g_ad_slab) (void)hipFree(g_ad_slab);
    g_ad_slab = nullptr; g_ad_slab_bytes = 0; g_ad_sig.clear();
    if (g_ad_tab) (void)hipFree(g_ad_tab);
    g_ad_tab = nullptr;
}

// dual array of ncomp components over the box of b (16 bytes per entry, the same padding as the library's arrays) out of the
// level's slab, filled with (src, 0) when src is given; the returned pointer is typed double* because BlkView is (the kernels see
// it as Dual*).  Measuring pass: only the size is added up.
static int ad_array(Block* b, AdBlock& a, double** field, const double* src, int ncomp)
{
    const size_t n = (size_t)b->v.nbox * ncomp;
    const size_t bytes = ((n + 32) * 16 + 255) & ~(size_t)255;
    if (g_ad_measure) { g_ad_bump += bytes; *field = nullptr; return 0; }
    if (g_ad_bump + bytes > g_ad_slab_bytes) return fail("forward mode: the slab of dual arrays is too small (internal error)");
    char* raw = g_ad_slab + g_ad_bump;
    g_ad_bump += bytes;
    a.init.push_back(AdInit{raw, src ? src - ADF_PAD0 : nullptr, n, (n + 32) * 16});
    *field = (double*)(raw + (size_t)ADF_PAD0 * 16);
    return 0;
}

// lays the dual arrays of every block of the level out (measuring pass or in the slab)
static int ad_layout(int level, bool viscous)
{
    return for_level(level, [&](Block* b) {
        AdBlock& a = g_ad[b];
        a.v = b->v;
        a.init.clear();
        BlkView& v = a.v;
        const BlkView& p = b->v;
        // active arrays (the seed kernel fills w; the evaluation writes the rest)
        if (ad_array(b, a, &v.w, nullptr, p.nw) || ad_array(b, a, &v.p, nullptr, 1) || ad_array(b, a, &v.rlv, p.rlv, 1) ||
            ad_array(b, a, &v.rev, p.rev, 1) || ad_array(b, a, &v.dw, nullptr, p.nw) || ad_array(b, a, &v.fw, nullptr, 5) ||
            ad_array(b, a, &v.dtl, nullptr, 1) || ad_array(b, a, &v.radI, nullptr, 1) || ad_array(b, a, &v.radJ, nullptr, 1) ||
            ad_array(b, a, &v.radK, nullptr, 1) || ad_array(b, a, &v.ss, p.ss, 1) || ad_array(b, a, &v.scratch, nullptr, 2))
            return 1;
        if (viscous && ad_array(b, a, &v.grad, nullptr, 12)) return 1;
        // passive arrays: value = the library's, derivative 0.  The geometry (x, sI/sJ/sK, vol, volRef, d2wall, dI/dJ/dK) is read by the
        // dual kernels as plain doubles out of the library's own arrays (blkview_def.h: ADF_GEOM), so it has no dual copy
        if (ad_array(b, a, &v.gamma, p.gamma, 1)) return 1;
        v.aa = nullptr; v.wn = v.pn = v.w1 = v.p1 = v.wr = nullptr; v.sFace = nullptr;
        // face arrays of the turbulence boundary treatment
        const size_t nf[3] = {(size_t)p.je * p.ke, (size_t)p.ie * p.ke, (size_t)p.ie * p.je};
        for (int f6 = 0; f6 < 6; ++f6)
            for (int which = 0; which < 2; ++which) {
                double** dst = &(which ? v.bvt : v.bmt)[f6];
                if (!(which ? p.bvt : p.bmt)[f6]) { *dst = nullptr; continue; }
                const size_t bytes = (nf[f6 / 2] * 16 + 255) & ~(size_t)255;
                if (g_ad_measure) { g_ad_bump += bytes; continue; }
                if (g_ad_bump + bytes > g_ad_slab_bytes) return fail("forward mode: the slab of dual arrays is too small (internal error)");
                char* raw = g_ad_slab + g_ad_bump;
                g_ad_bump += bytes;
                a.init.push_back(AdInit{raw, nullptr, nf[f6 / 2], nf[f6 / 2] * 16});
                *dst = (double*)raw;
            }
        return 0;
    });
}

// sync = false (the matrix-free products in the enqueue-only mode): the host waits only where the slab had to be laid out
static int ad_prepare(int level, bool sync = true)
{
    if (ensure_table(level)) return 1;
    const int maxnn = g_tab_size[level];
    const bool viscous = g_opts.equations != ADFLOW_EULER;
    // the layout the slab must have: level, model, and per block its identity, box, variables and optional arrays
    std::vector<long> sig = {level, viscous ? 1 : 0, maxnn};
    int rc = for_level(level, [&](Block* b) {
        if (!b->geom_uploaded) return fail("geometry of a level-%d block has not been uploaded", level);
        if (viscous) block_face_vectors(b);
        const BlkView& p = b->v;
        sig.push_back((long)(uintptr_t)b); sig.push_back(p.nbox); sig.push_back(p.nw);
        sig.push_back((p.d2wall ? 1 : 0) | (p.dI ? 2 : 0) | (p.bmt[0] ? 4 : 0));
        sig.push_back((long)(uintptr_t)p.w); sig.push_back((long)(uintptr_t)p.x);
        return 0;
    });
    if (rc) return rc;
    if (!g_ad_slab || sig != g_ad_sig) {
        ad_drop();
        g_ad_measure = true; g_ad_bump = 0;
        rc = ad_layout(level, viscous);
        g_ad_measure = false;
        if (rc) return rc;
        const size_t need = g_ad_bump + 4096;
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB < need + ((size_t)64 << 20))
            return fail("forward mode needs %.2f GB for the dual copies of the level's arrays, %.2f GB are free on the device", need / 1.e9, freeB / 1.e9);
        HIPCHK(hipMalloc((void**)&g_ad_slab, need));
        g_ad_slab_bytes = need;
        g_ad_bump = 0;
        g_ad.clear();
        if (ad_layout(level, viscous)) { ad_drop(); return 1; }
        std::vector<BlkView> h(maxnn + 1);
        memset(h.data(), 0, sizeof(BlkView) * h.size());
        for (auto& kv : g_blocks)
            if (std::get<0>(kv.first) == level && std::get<1>(kv.first) == 1) h[std::get<2>(kv.first)] = g_ad[kv.second].v;
        HIPCHK(hipMalloc((void**)&g_ad_tab, sizeof(BlkView) * h.size()));
        HIPCHK(hipMemcpyAsync(g_ad_tab, h.data(), sizeof(BlkView) * h.size(), hipMemcpyHostToDevice, g_stream));
        g_ad_sig = sig;
        sync = true;                   // (h is read by the copy above)
    }
    // values of this call: the passive arrays and the frozen closures from the library's arrays, zero elsewhere
    for (auto& kv : g_ad)
        for (const AdInit& q : kv.second.init) {
            if (q.src) ad_launch_from_real(q.src, q.dst, (long)q.n, g_stream);
            else HIPCHK(hipMemsetAsync(q.dst, 0, q.zeroBytes, g_stream));
        }
    if (sync) HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

// the device table of the snapshot request: per block slot of the level its snapshot array and its scaled reference residual
static int snap_request_begin(int level, const JacSpec& J)
{
    if (ensure_table(level)) return 1;
    const int n = g_tab_size[level] + 1;
    std::vector<SnapSlot> h((size_t)n, SnapSlot{nullptr});
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level && std::get<1>(kv.first) == 1) h[std::get<2>(kv.first)] = SnapSlot{kv.second->snap};
    if (g_snapreq.devSlots < n) {
        if (g_snapreq.dev) (void)hipFree(g_snapreq.dev);
        g_snapreq.dev = nullptr; g_snapreq.devSlots = 0;
        HIPCHK(hipMalloc((void**)&g_snapreq.dev, sizeof(SnapSlot) * (size_t)n));
        g_snapreq.devSlots = n;
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    HIPCHK(hipMemcpy(g_snapreq.dev, h.data(), sizeof(SnapSlot) * (size_t)n, hipMemcpyHostToDevice));
    g_snapreq.level = level; g_snapreq.col = 0; g_snapreq.l0 = J.lStart; g_snapreq.n = J.nState;
    g_snapreq.turbScale = g_opts.turbResScale;
    g_snapreq.on = true;
    return 0;
}
namespace {
struct SnapRequestGuard { ~SnapRequestGuard() { g_snapreq.on = false; } };
// the switches of the preconditioner matrix (adjointUtils.F90:176-191) for one assembly, handed back on every exit
struct PcSwitchGuard {
    const adflow_opts opts;
    const int lumped;
    explicit PcSwitchGuard(bool pc) : opts(g_opts), lumped(g_lumped)
    {
        if (!pc) return;
        g_lumped = 1;
        g_opts.acousticScaleFactor = 1.0;
        g_opts.orderTurb = 1;                                           // constants::firstOrder
    }
    ~PcSwitchGuard() { g_opts = opts; g_lumped = lumped; }
};
}  // namespace

// who: the entry that reports; ad: what it appends where forward mode is the reason ("(useAD)", or nothing for the matrix-free entries)
static int jac_check_args(int level, unsigned flags, double delta, const char* who = "fd_jacobian", const char* ad = "(useAD)")
{
    if (flags & ~(ADFLOW_JAC_PC | ADFLOW_JAC_FROZEN_TURB | ADFLOW_JAC_TURB_ONLY | ADFLOW_JAC_VISC_PC | ADFLOW_JAC_USE_AD | ADFLOW_JAC_APPROX_SA))
        return fail("%s: unknown flags 0x%x", who, flags);
    const bool useAD = (flags & ADFLOW_JAC_USE_AD) != 0;
    if (!useAD && !(delta > 0.0)) return fail("%s: delta must be positive", who);     // forward mode has no step size
    if (useAD) {
        // forward-mode seeds instead of perturbations (adjointUtils.F90:227-409): kernels on dual numbers, blocks at rest
        if (!level_at_rest(level)) return fail("%s%s: moving blocks are not linearised (grid velocities)", who, ad);
        if (!g_act.empty()) return fail("%s%s: actuator regions are not linearised", who, ad);
        if (g_bc_callback) return fail("%s%s: a host boundary-condition hook cannot be linearised", who, ad);
        if (g_turb_bc_callback && g_opts.equations == ADFLOW_RANS && !(flags & ADFLOW_JAC_FROZEN_TURB))
            return fail("%s%s: a host turbulence boundary-condition hook cannot be linearised", who, ad);
    }
    if (level != g_opts.groundLevel) return fail("%s: level %d is not the ground level %d (setupStateResidualMatrix sets both)", who, level, g_opts.groundLevel);
    if ((flags & ADFLOW_JAC_TURB_ONLY) && g_opts.equations != ADFLOW_RANS) return fail("%s: ADFLOW_JAC_TURB_ONLY needs the RANS equations", who);
    if ((flags & ADFLOW_JAC_TURB_ONLY) && (flags & ADFLOW_JAC_FROZEN_TURB)) return fail("%s: TURB_ONLY and FROZEN_TURB exclude each other", who);
    return 0;
}

// per block: reference state and residual, the stencil blocks, the snapshots of the nColour evaluations of one state variable
static int jac_storage(int level, const JacSpec& J)
{
    const int ncomp = J.nStencil * J.nState * J.nState, nsnap = J.cn * J.nState;
    return for_level(level, [&](Block* b) {
        if (!b->wref) {
            if (alloc_arr(b, &b->wref, b->v.nw) || alloc_arr(b, &b->dwref, 6)) return 1;
        }
        // (no memset of the blocks: k_fd_scatter stores every entry of every owned row, and only owned rows are ever read)
        auto resize = [&](void** raw, double** arr, int* have, int want) {
            if (*have == want) return 0;
            if (*raw) HIPCHK(hipFree(*raw));
            *raw = nullptr; *arr = nullptr; *have = 0;
            HIPCHK(hipMalloc(raw, (size_t)b->v.nbox * want * sizeof(double) + 256));
            *arr = (double*)*raw + ADF_PAD0;
            *have = want;
            return 0;
        };
        if (resize(&b->jac_raw, &b->jac, &b->jac_ncomp, ncomp)) return 1;
        return resize(&b->snap_raw, &b->snap, &b->snap_ncomp, nsnap);
    });
}

// The coloured sweep of both assemblies: for every state variable l and colour, the seed launch puts the state of the evaluation in place
// (PLAIN: wref + delta on component l of the cells of the colour; DUAL: seed = 1 there, halos included), block_res_state runs, and the
// scaled residual (its derivative) is the snapshot of the colour; once per variable the snapshots are scattered into the column l of
// every stencil block (PLAIN: as finite differences against dwref).  The reference loops colours outside and state variables inside;
// every (colour, variable) evaluation is independent, so the loops are exchanged here: the nColour evaluations of one variable are
// kept (dense) and scattered into the blocks together.
// oneComponent: inside the sweep of one state variable over the colours only that component of the state changes; the others are
// written at its first colour only (the caller says when that is allowed)
static int coloured_sweep(const Launchers& M, int level, const JacSpec& J, unsigned resFlags, bool turbBC, bool viscPC, bool oneComponent,
                          double delta)
{
    SnapRequestGuard snapGuard;        // no exit leaves the request standing
    // (the seed kernel reads only options of kp that no flag of the evaluation changes)
    const KParams kp = res_kparams(level, resFlags);
    // the marching kernels of the preconditioner matrix write the snapshot of an evaluation themselves (KParams::snapTab): not with
    // actuator regions (their sources are added to dw behind the core).  The plan is that of the KParams and flags every coloured
    // evaluation below builds again.  The launchers report what they wrote (adf_note_snap): a host prediction that turns out wrong
    // is an error instead of a matrix built from stale memory
    const FlowPlan P = plan_flow(flow_facts(level, kp, visc_approx(M, resFlags, viscPC), false, M.dual, resFlags));
    const int need = ((resFlags & ADFLOW_RES_FLOW) ? 1 : 0) | ((resFlags & ADFLOW_RES_TURB) ? 2 : 0);
    const bool snapInMarch = g_act.empty() && (!(need & 1) || P.flowSnapInMarch) && (!(need & 2) || P.turbSnapInMarch);
    if (snapInMarch && snap_request_begin(level, J)) return 1;
    for (int l = J.lStart; l < J.lStart + J.nState; ++l) {
        for (int col = 0; col < J.cn; ++col) {
            g_snapreq.col = col;
            for_level(level, [&](Block* b) {
                if (M.dual) ad_launch_seed_closures(b->v, g_ad[b].v, l, col, J, kp, g_stream, oneComponent && col > 0);
                else launch_fd_state_closures(b->v, b->wref, l, col, J, delta, kp, g_stream, oneComponent && col > 0);
                return 0;
            });
            g_snap_done = 0;
            if (block_res_state_enqueue(M, level, resFlags, turbBC, viscPC, true)) return 1;
            if (snapInMarch && (g_snap_done & need) != need)
                return fail("fd_jacobian: the marching kernels were expected to write the snapshot of the evaluation (need %d, written %d)", need, g_snap_done);
            if (!snapInMarch)
                for_level(level, [&](Block* b) {
                    double* snap = b->snap + (size_t)col * J.nState * b->v.nbox;
                    if (M.dual) ad_launch_snap(b->v, g_ad[b].v.dw, snap, J, g_opts.turbResScale, g_stream);
                    else launch_fd_snap(b->v, snap, J, g_opts.turbResScale, g_stream);
                    return 0;
                });
        }
        for_level(level, [&](Block* b) {
            launch_fd_scatter(b->v, b->snap, b->jac, l, J, M.dual ? nullptr : b->dwref, M.dual ? 0.0 : 1.0 / delta, g_stream);
            return 0;
        });
    }
    return 0;
}

int adflow_gpu_fd_jacobian(int level, unsigned flags, double delta)
{
    if (need_ready() || jac_check_args(level, flags, delta)) return 1;
    const bool useAD = (flags & ADFLOW_JAC_USE_AD) != 0;
    const Launchers& M = useAD ? DUAL : PLAIN;
    const bool rans = g_opts.equations == ADFLOW_RANS;
    JacSpec J;
    jac_spec(flags & ~(ADFLOW_JAC_USE_AD | ADFLOW_JAC_APPROX_SA), rans || g_opts.equations == ADFLOW_NS, rans, &J);
    if (jac_storage(level, J)) return 1;
    g_jac_valid = false;

    // whalo2(1, 1, nw, T, T, T) (adjointUtils.F90:113)
    if (g_comm.count(std::make_pair(level, 2)))
        if (halo_exchange_enqueue(level, 1, rans ? 6 : 5, 1, 1, 2)) return 1;

    const bool pc = (flags & ADFLOW_JAC_PC) != 0;
    PcSwitchGuard switches(pc);
    unsigned resFlags = 0;
    if (!(flags & ADFLOW_JAC_TURB_ONLY)) resFlags |= ADFLOW_RES_FLOW;
    // frozenTurb: equations = NSEquations (adjointUtils.F90:218-222) -- no turbulence boundary conditions, no SA residual; the eddy
    // viscosity is still recomputed from nuTilde because eddyModel stays set (turbUtils.F90:604-612)
    const bool turbBC = rans && !(flags & ADFLOW_JAC_FROZEN_TURB);
    if (turbBC) resFlags |= ADFLOW_RES_TURB;
    if (turbBC && (flags & ADFLOW_JAC_APPROX_SA)) resFlags |= ADFLOW_RES_APPROX_SA;     // FormJacobianANK:1978, FormJacobianANKTurb:2364
    int rc = 0;
    if (pc) {
        resFlags |= ADFLOW_RES_DISS_APPROX | ADFLOW_RES_VISC_APPROX;     // dissApprox = viscApprox = lumpedDiss
        // referenceShockSensor on the unperturbed state (adjointUtils.F90:258-260): the sensor is not linearised
        rc = reference_shock_sensor_enqueue(level);
    }
    // What differs from a full rewrite of the state at every colour is the content of halos BEFORE the boundary conditions of the
    // evaluation overwrite them (the output of the previous evaluation instead of the reference state): face halos are functions of
    // the interior alone, but the halo cells along block EDGES are written by one subface from what another left there, in an order
    // -- so the shortcut is taken for the preconditioner matrix, whose 7-point stencils never reach an edge halo, and not with a host hook
    // (... nor for viscPC, whose full viscous flux reads edge and corner halos through its 27-point stencil: round-5 advisor)
    const bool viscPC = (flags & ADFLOW_JAC_VISC_PC) != 0;
    const bool oneComponent = pc && !viscPC && !g_bc_callback && !g_turb_bc_callback;

    bool haveRef = false;           // wref holds the reference state: an error further down still puts the state back
    if (useAD) {
        if (!rc) rc = ad_prepare(level);
    } else {
        // setFDReference (adjointUtils.F90:1971-2024): reference residual, then the reference state INCLUDING the halos the boundary
        // conditions just wrote
        if (!rc) rc = block_res_state_enqueue(PLAIN, level, resFlags, turbBC, viscPC);
        if (!rc) rc = for_level(level, [&](Block* b) {
            launch_fd_copy(b->v, b->wref, b->v.w, b->v.nw, g_stream);
            launch_fd_extract(b->v, b->dwref, b->jac, -1, 0, J, 0.0, g_opts.turbResScale, g_stream);
            return 0;
        });
        haveRef = !rc;
    }
    if (!rc) rc = coloured_sweep(M, level, J, resFlags, turbBC, viscPC, oneComponent, delta);
    if (useAD) {
        if (!rc) rc = sync_and_check();
        else (void)hipStreamSynchronize(g_stream);
        if (!g_ad_cache || rc) ad_drop();
    } else if (haveRef) {
        // resetFDReference (adjointUtils.F90:2026-2058): w back, dw = the (scaled) reference residual -- after a sweep that stopped
        // half way the state alone: the level must not keep a perturbed one (the error text of the failed call is kept)
        for_level(level, [&](Block* b) {
            launch_fd_state(b->v, b->wref, 0, -1, J, 0.0, g_stream);
            if (!rc) launch_fd_extract(b->v, b->dwref, b->jac, -2, 0, J, 0.0, g_opts.turbResScale, g_stream);
            b->ss_valid = false;
            b->etot_consistent = false;
            return 0;
        });
        if (rc) (void)hipStreamSynchronize(g_stream);
    }
    if (rc) return rc;
    g_jac = J;
    g_jac_level = level;
    g_jac_valid = true;
    return useAD ? 0 : sync_and_check();        // (forward mode synchronised before it decided about its slab)
}

int adflow_gpu_release_workspace(int64_t* bytes)
{
    if (need_ready()) return 1;
    if (g_stream) HIPCHK(hipStreamSynchronize(g_stream));
    const int64_t jm = jm_release();
    const int64_t wi = wi_drop_all();
    if (bytes) *bytes = (int64_t)g_ad_slab_bytes + jm + wi;
    ad_drop();
    return 0;
}

int adflow_gpu_selftest_math(int which, const double* x, const double* a, int64_t n, double* y, double* dy)
{
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    if (which < 0 || which > 7 || n < 0 || !x || !a || !y || !dy) return fail("selftest_math: bad arguments");
    if (n == 0) return 0;
    double* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, sizeof(double) * 5 * (size_t)n));          // x, a, y, (value, derivative)
    int rc = 0;
    if (hipMemcpy(d, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + n, a, sizeof(double) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail("selftest_math: upload failed");
    if (!rc) {
        ad_launch_selftest_math(which, d, d + n, (long)n, d + 2 * n, d + 3 * n, g_stream);
        if (hipStreamSynchronize(g_stream) != hipSuccess || hipMemcpy(y, d + 2 * n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(dy, d + 3 * n, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail("selftest_math: kernel or download failed");
    }
    (void)hipFree(d);
    return rc;
}

int adflow_gpu_jacobian_info(int32_t* nState, int32_t* nStencil, int32_t* stencil)
{
    if (!g_jac_valid) return fail("jacobian_info: no assembled Jacobian (call adflow_gpu_fd_jacobian first)");
    if (nState) *nState = g_jac.nState;
    if (nStencil) *nStencil = g_jac.nStencil;
    if (stencil)
        for (int s = 0; s < g_jac.nStencil; ++s)
            for (int d = 0; d < 3; ++d) stencil[(size_t)d * g_jac.nStencil + s] = g_jac.st[s][d];
    return 0;
}

int adflow_gpu_download_jacobian(int nn, int level, int sps, double* blocks)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (!g_jac_valid || !b->jac) return fail("download_jacobian: no assembled Jacobian on block (%d,%d,%d)", nn, level, sps);
    if (!blocks) return fail("download_jacobian: blocks is NULL");
    BlkView& v = b->v;
    int rc = copy_box(b, b->jac, blocks, b->jac_ncomp, 2, v.nx, 2, v.ny, 2, v.nz, false);
    if (rc) return rc;
    return sync_and_check();
}

int adflow_gpu_download_jacobian_rows(int nn, int level, int sps, double* rows)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (!g_jac_valid || !b->jac) return fail("download_jacobian_rows: no assembled Jacobian on block (%d,%d,%d)", nn, level, sps);
    if (!rows) return fail("download_jacobian_rows: rows is NULL");
    const BlkView& v = b->v;
    const int nS = g_jac.nState, nSt = g_jac.nStencil;
    if (nS * nS >= 37) return fail("download_jacobian_rows: nState = %d exceeds the tile of the transposition kernel", nS);
    const size_t perPlane = (size_t)v.nx * v.ny * nSt * nS * nS;          // doubles of one k plane of rows
    int nk = (int)std::max<size_t>(1, ((size_t)128 << 20) / (perPlane * 8));   // slabs of <= 128 MB on the device
    if (nk > v.nz) nk = v.nz;
    double* d_out = nullptr;
    HIPCHK(hipMalloc((void**)&d_out, perPlane * nk * 8));
    for (int k0 = 0; k0 < v.nz; k0 += nk) {
        const int n = std::min(nk, v.nz - k0);
        launch_jac_rows(v, b->jac, d_out, nS, nSt, k0 + 2, n, g_stream);
        if (hipMemcpyAsync(rows + perPlane * k0, d_out, perPlane * n * 8, hipMemcpyDeviceToHost, g_stream) != hipSuccess ||
            hipStreamSynchronize(g_stream) != hipSuccess) {
            (void)hipFree(d_out);
            return fail("download_jacobian_rows: copy of the planes %d.. failed", k0 + 2);
        }
    }
    HIPCHK(hipFree(d_out));
    return sync_and_check();
}

}  // extern "C"

// ------------------------------------------------------------ halo exchange
namespace {

struct LevelDims { int nx, ny, nz; };
std::map<int, LevelDims> g_tab_dims;                   // largest block extents of a level (grid of the batched launches)

int ensure_table(int level)
{
    if (g_tab.count(level)) return 0;
    int maxnn = 0;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level) maxnn = std::max(maxnn, std::get<2>(kv.first));
    if (maxnn == 0) return fail("no block registered on level %d", level);
    std::vector<BlkView> h(maxnn + 1);
    memset(h.data(), 0, sizeof(BlkView) * h.size());
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level && std::get<1>(kv.first) == 1) h[std::get<2>(kv.first)] = kv.second->v;
    long off = 0;                     // PETSc vector order: block nn ascending (NKSolvers.F90:1240-1253)
    for (auto& v : h) {
        v.vecOff = off;
        off += (long)v.nx * v.ny * v.nz * v.nw;
    }
    BlkView* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, sizeof(BlkView) * h.size()));
    HIPCHK(hipMemcpy(d, h.data(), sizeof(BlkView) * h.size(), hipMemcpyHostToDevice));
    g_tab[level] = d;
    g_tab_size[level] = maxnn;
    LevelDims ld = {0, 0, 0};
    for (auto& v : h) { ld.nx = std::max(ld.nx, v.nx); ld.ny = std::max(ld.ny, v.ny); ld.nz = std::max(ld.nz, v.nz); }
    g_tab_dims[level] = ld;
    return 0;
}

// level-batched pointwise launches: device block table + the largest block extents of the level
int level_tab(int level, LevelTab* t)
{
    if (ensure_table(level)) return 1;
    const LevelDims& ld = g_tab_dims[level];
    t->tab = g_tab[level]; t->n = g_tab_size[level]; t->nx = ld.nx; t->ny = ld.ny; t->nz = ld.nz;
    return 0;
}

int time_step_level(int level, const KParams& kp)
{
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_time_step_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, g_stream);
    // the NS / RANS kernel also leaves the entropy sensor in ss -- but not in a dissApprox pass (frozen sensor kept)
    const bool wrote_ss = kp.viscous && !kp.dissApprox;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level) kv.second->ss_valid = wrote_ss;
    return 0;
}

// implicit residual averaging of every block of the level (one launch per direction)
// scaleDtl != 0: dw enters as scaleDtl dtl dw (the stage scaling of the Runge-Kutta smoother): folded into the first sweep when every
// block of the level has an i sweep, a pointwise pass in front otherwise
int res_averaging_level(int level, const KParams& kp, double scaleDtl)
{
    if (ensure_table(level)) return 1;
    const LevelDims& ld = g_tab_dims[level];
    bool fold = (scaleDtl != 0.0);
    for_level(level, [&](Block* b) { fold = fold && b->v.nx > 1; return 0; });
    if (scaleDtl != 0.0 && !fold) launch_scale_dw_level(g_tab[level], g_tab_size[level], ld.nx, ld.ny, ld.nz, scaleDtl, 0, g_stream);
    launch_res_averaging_level(g_tab[level], g_tab_size[level], ld.nx, ld.ny, ld.nz, kp, g_stream, fold ? scaleDtl : 0.0);
    return 0;
}

// tile table of the k-marching Euler kernel for every block of a level.  The
// dispatcher places workgroup p on XCD p % 8 (MI355X_MICROARCH.md): entry p holds
// the tile  (p % 8) * ceil(n/8) + p / 8  of the natural order (i-tile fastest, then
// j, k, block) so that each XCD owns one contiguous slab and j/k-neighbouring tiles
// share its 4 MiB L2.
}  // namespace

// workgroups of a marching kernel resident at a time: two per CU (256 VGPRs, <= 80 KB of LDS each)
void adf_note_rvec(int bits) { g_rvec_done |= bits; }
int adf_fail(const char* what) { return fail("%s", what); }
void adf_note_snap(int bits) { g_snap_done |= bits; }

int adf_round_size()
{
    if (g_num_cus <= 0) {
        hipDeviceProp_t prop;
        if (g_device >= 0 && hipGetDeviceProperties(&prop, g_device) == hipSuccess) g_num_cus = prop.multiProcessorCount;
        if (g_num_cus <= 0) g_num_cus = 256;
    }
    return 2 * g_num_cus;
}

namespace {

// Launch order of T work items that run in rounds of W resident workgroups: slot p of the table -> item (or -1 = empty slot).  Every
// round occupies Wp = W rounded up to a multiple of 8 slots, so that slot p is dispatched to XCD p % 8 in every round whatever the CU
// count (round-3 advisor finding: with W % 8 != 0 the plain (p % W) / 8, (p % W) % 8 decode dropped items); inside a round XCD x takes
// the x-th contiguous eighth of the round's items.  Checked: every item exactly once.
int round_order(int T, int W, std::vector<int>* out)
{
    if (W < 1) W = 1;
    const int Wp = (W + 7) / 8 * 8, rounds = (T + W - 1) / W;
    out->assign((size_t)rounds * Wp, -1);
    long seen = 0;
    for (int q = 0; q < rounds; ++q) {
        const int nIn = std::min(W, T - q * W), per = (nIn + 7) / 8;
        for (int pr = 0; pr < Wp; ++pr) {
            const int s = pr / 8, x = pr % 8;
            if (s < per && x * per + s < nIn) { (*out)[(size_t)q * Wp + pr] = q * W + x * per + s; ++seen; }
        }
    }
    if (seen != T) return fail("round_order: %ld of %d work items placed (W = %d)", seen, T, W);
    std::vector<char> hit((size_t)T, 0);
    for (int e : *out)
        if (e >= 0) { if (hit[e]) return fail("round_order: item %d placed twice", e); hit[e] = 1; }
    return 0;
}

int ensure_tiles(int level)
{
    if (g_tiles.count(level)) return 0;
    if (ensure_table(level)) return 1;
    std::vector<int4> nat;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level || std::get<1>(kv.first) != 1) continue;
        int ntx, nty, ntz;
        euler_march_tiles(kv.second->v, &ntx, &nty, &ntz);
        for (int tz = 0; tz < ntz; ++tz)
            for (int ty = 0; ty < nty; ++ty)
                for (int tx = 0; tx < ntx; ++tx) {
                    int4 t;
                    t.x = std::get<2>(kv.first); t.y = tx; t.z = ty; t.w = tz;
                    nat.push_back(t);
                }
    }
    // workgroup p runs on XCD p % 8.  xcd_tiles = 1: XCD x takes the x-th contiguous eighth of the whole table; 2 (default): of every
    // ROUND of resident workgroups (adf_round_size), so that at any time the eight XCDs work on neighbouring tiles of one block
    // (no measurable difference to 1 on the north-star mesh, profiles/r03_d_xcd_round_ab.txt; it keeps the working set of a round
    // compact when a level holds many blocks)
    const int n = (int)nat.size();
    const int W = (g_xcd_tiles >= 2) ? adf_round_size() : ((n + 7) / 8) * 8;
    std::vector<int> ord;
    if (g_xcd_tiles) {
        if (round_order(n, W, &ord)) return 1;
    } else {
        ord.resize(n);
        for (int p = 0; p < n; ++p) ord[p] = p;
    }
    std::vector<int4> phys(ord.size());
    for (size_t p = 0; p < ord.size(); ++p) {
        if (ord[p] >= 0) phys[p] = nat[ord[p]];
        else { phys[p].x = -1; phys[p].y = phys[p].z = phys[p].w = 0; }
    }
    while (!phys.empty() && phys.back().x < 0) phys.pop_back();
    int4* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, sizeof(int4) * phys.size()));
    HIPCHK(hipMemcpy(d, phys.data(), sizeof(int4) * phys.size(), hipMemcpyHostToDevice));
    g_tiles[level] = std::make_pair(d, (int)phys.size());
    return 0;
}

// Chunk table of the fused gradient + viscous march (k_visc_gf).  A column = (block, 60-column tile, 3-row tile); every column is cut
// into chunks of k planes, one workgroup per chunk, and a workgroup costs (planes + ~1.5 warm-up planes).  The device keeps
// W = 2 x CUs workgroups of this kernel resident and dispatches them in launch order, so the launch runs in "rounds" of W workgroups
// of about equal duration: with N columns x c chunks just above a multiple of W the last round is almost empty (north-star mesh:
// 1032 columns x 2 chunks = 4.03 rounds = the time of 5).  Here the NUMBER of chunks is chosen as a whole number of rounds, columns
// get c or c+1 chunks, the chunks are launched longest first (every round holds chunks of one length), and within a round
// workgroup p = 8 s + x takes the x-th contiguous eighth of the round's chunks, so that XCD x (which receives the workgroups
// p % 8 == x) works on neighbouring tiles.  Entry: x = block slot (-1: empty), y = bx | by << 16, z = first plane, w = last plane.
// R = produced cell rows per workgroup (3: k_visc_gf, 4: k_sa_march), warm = planes a chunk costs beyond its own, reach = cells the
// stencil of a produced cell reaches (the interior / boundary partition); all / in / bd: the three tables
static int build_chunk_tables(int level, int R, double warm, int reach, std::pair<int4*, int>* all, std::pair<int4*, int>* in_,
                              std::pair<int4*, int>* bd_, int wgPerCU = 2)
{
    if (ensure_table(level)) return 1;
    struct Col { int slot, bx, by, nz, nx, ny; };
    std::vector<Col> cols;
    long planes = 0;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level || std::get<1>(kv.first) != 1) continue;
        const BlkView& v = kv.second->v;
        const int gx = (v.nx + 59) / 60, gy = (v.ny + R - 1) / R;
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx) { cols.push_back(Col{std::get<2>(kv.first), bx, by, v.nz, v.nx, v.ny}); planes += v.nz; }
    }
    const int N = (int)cols.size();
    *all = *in_ = *bd_ = std::make_pair((int4*)nullptr, 0);
    if (N == 0) return 0;
    const int W = adf_round_size() * wgPerCU / 2;       // resident workgroups of the kernel: wgPerCU per CU
    const int kmin = 8;
    // chunks of a column for a total of T chunks: proportional to its planes (largest remainder), at least 1, at most nz / kmin
    auto split = [&](long T, std::vector<int>& c) {
        c.assign(N, 1);
        long used = 0;
        std::vector<std::pair<double, int>> rem(N);
        for (int q = 0; q < N; ++q) {
            const double want = (double)T * cols[q].nz / (double)planes;
            const int cmax = std::max(1, cols[q].nz / kmin);
            c[q] = std::min(cmax, std::max(1, (int)want));
            rem[q] = std::make_pair(want - c[q], q);
            used += c[q];
        }
        std::sort(rem.begin(), rem.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first > b.first; });
        for (int q = 0; q < N && used < T; ++q) {
            const int id = rem[q].second;
            if (c[id] < std::max(1, cols[id].nz / kmin)) { ++c[id]; ++used; }
        }
    };
    auto makespan = [&](const std::vector<int>& c) {
        std::vector<int> len;
        for (int q = 0; q < N; ++q)
            for (int e = 0; e < c[q]; ++e) len.push_back((cols[q].nz + c[q] - 1 - e) / c[q]);
        std::sort(len.begin(), len.end(), [](int a, int b) { return a > b; });
        double t = 0.0;
        for (size_t q = 0; q < len.size(); q += W) t += len[q] + warm;
        return t;
    };
    std::vector<int> best;
    if (!g_gf_nofit) {
        double tbest = 1.e300;
        const long Tmax = std::max<long>(N, planes / kmin);
        for (long m = 1; m * W <= Tmax + W; ++m) {
            std::vector<int> c;
            split(m * W, c);
            const double t = makespan(c);
            if (t < tbest - 1.e-9) { tbest = t; best = c; }
            if (m > 64) break;
        }
        // a level much smaller than the device: one chunk per column unless splitting fills more of it
        std::vector<int> one(N, 1);
        if (makespan(one) < tbest) best = one;
    } else {
        best.resize(N);
        const int L = g_march_kch > 0 ? g_march_kch : 32;
        for (int q = 0; q < N; ++q) best[q] = (cols[q].nz + L - 1) / L;
    }
    struct Chunk { int col, k0, k1; };
    std::vector<Chunk> ch;
    for (int q = 0; q < N; ++q) {
        int k = 2;
        for (int e = 0; e < best[q]; ++e) {
            const int len = (cols[q].nz + best[q] - 1 - e) / best[q];
            if (len <= 0) continue;
            ch.push_back(Chunk{q, k, k + len - 1});
            k += len;
        }
    }
    // longest first; chunks of one length in (block, k, row tile, column tile) order
    std::stable_sort(ch.begin(), ch.end(), [&](const Chunk& a, const Chunk& b) {
        const int la = a.k1 - a.k0, lb = b.k1 - b.k0;
        if (la != lb) return la > lb;
        if (cols[a.col].slot != cols[b.col].slot) return cols[a.col].slot < cols[b.col].slot;
        if (a.k0 != b.k0) return a.k0 < b.k0;
        return a.col < b.col;
    });
    // round-ordered device table of a chunk list
    auto make_table = [&](const std::vector<Chunk>& list, std::pair<int4*, int>* out) -> int {
        const int T = (int)list.size();
        std::vector<int> ord;
        if (round_order(T, W, &ord)) return 1;
        std::vector<int4> phys(ord.size());
        for (size_t p = 0; p < ord.size(); ++p) {
            const int e = ord[p];
            int4 tt;
            if (e >= 0) {
                const Col& c = cols[list[e].col];
                tt.x = c.slot; tt.y = c.bx | (c.by << 16); tt.z = list[e].k0; tt.w = list[e].k1;
            } else { tt.x = -1; tt.y = tt.z = tt.w = 0; }
            phys[p] = tt;
        }
        int n = (int)phys.size();                              // trailing empty entries are not launched
        while (n > 0 && phys[n - 1].x < 0) --n;
        int4* d = nullptr;
        HIPCHK(hipMalloc((void**)&d, sizeof(int4) * std::max(n, 1)));
        if (n > 0) HIPCHK(hipMemcpy(d, phys.data(), sizeof(int4) * n, hipMemcpyHostToDevice));
        *out = std::make_pair(d, n);
        return 0;
    };
    if (make_table(ch, all)) return 1;
    // the same chunks in two tables for the evaluation split around the halo exchange: "interior" = the produced cells (columns
    // 2+60 bx .., rows 2+R by .., planes k0 .. k1) and their stencil (+-reach) lie inside the owned range
    std::vector<Chunk> in, bd;
    for (const Chunk& c : ch) {
        const Col& q = cols[c.col];
        const int il = q.nx + 1, jl = q.ny + 1, kl = q.nz + 1;
        const int ia = 2 + 60 * q.bx, ib_ = std::min(ia + 59, il), ja = 2 + R * q.by, jb_ = std::min(ja + R - 1, jl);
        const bool interior = (ia - reach >= 2 && ib_ + reach <= il && ja - reach >= 2 && jb_ + reach <= jl && c.k0 - reach >= 2 &&
                               c.k1 + reach <= kl);
        (interior ? in : bd).push_back(c);
    }
    if (make_table(in, in_) || make_table(bd, bd_)) return 1;
    return 0;
}

int ensure_gf_tiles(int level)
{
    if (g_gf_tiles.count(level)) return 0;
    std::pair<int4*, int> a, i, b;
    if (build_chunk_tables(level, 3, 1.5, 1, &a, &i, &b, 2)) return 1;
    g_gf_tiles[level] = a; g_gf_tiles_int[level] = i; g_gf_tiles_bnd[level] = b;
    return 0;
}

// chunk tables of the Spalart-Allmaras march: 60 columns x 4 rows, no warm-up plane beyond the window fill, stencil +-2
int ensure_sa_tiles(int level)
{
    if (g_sa_tiles.count(level)) return 0;
    std::pair<int4*, int> a, i, b;
    if (build_chunk_tables(level, 4, 0.5, 2, &a, &i, &b)) return 1;
    g_sa_tiles[level] = a; g_sa_tiles_int[level] = i; g_sa_tiles_bnd[level] = b;
    return 0;
}

int make_list_host(int level, const int32_t* blk, const int32_t* idx, int ld, int first, int n, std::vector<int>& hb,
                   std::vector<long>& ho)
{
    hb.resize(n);
    ho.resize(n);
    for (int t = 0; t < n; ++t) {
        const int nn = blk[first + t];
        Block* b = find_block(nn, level, 1);
        if (!b) return fail("comm pattern of level %d references unregistered block %d", level, nn);
        const int i = idx[first + t], j = idx[ld + first + t], k = idx[2 * ld + first + t];
        if (i < 0 || i > b->v.ib || j < 0 || j > b->v.jb || k < 0 || k > b->v.kb)
            return fail("comm pattern of level %d: cell (%d,%d,%d) outside block %d", level, i, j, k, nn);
        hb[t] = nn;
        ho[t] = b->v.idx(i, j, k);
    }
    return 0;
}

int upload_list(const std::vector<int>& hb, const std::vector<long>& ho, int** d_blk, long** d_off)
{
    const size_t n = hb.size();
    *d_blk = nullptr;
    *d_off = nullptr;
    if (n == 0) return 0;
    HIPCHK(hipMalloc((void**)d_blk, sizeof(int) * n));
    HIPCHK(hipMalloc((void**)d_off, sizeof(long) * n));
    HIPCHK(hipMemcpy(*d_blk, hb.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(*d_off, ho.data(), sizeof(long) * n, hipMemcpyHostToDevice));
    return 0;
}

int make_list(int level, const int32_t* blk, const int32_t* idx, int ld, int first, int n, int** d_blk, long** d_off)
{
    std::vector<int> hb;
    std::vector<long> ho;
    if (make_list_host(level, blk, idx, ld, first, n, hb, ho)) return 1;
    return upload_list(hb, ho, d_blk, d_off);
}

int build_comm(int level, int nLayers, CommPattern** out)
{
    auto it = g_comm.find(std::make_pair(level, nLayers));
    if (it == g_comm.end()) return fail("no %d-layer comm pattern registered for level %d", nLayers, level);
    CommPattern& cp = it->second;
    *out = &cp;
    if (ensure_table(level)) return 1;
    if (cp.built) return 0;
    const int nc = (int)cp.h_donorBlock.size();
    cp.local.n = nc;
    {
        // same-GPU copies: the (donor, halo) pairs are independent (donors are owned cells), so they are
        // re-ordered by halo address: consecutive lanes then write - and for 1-to-1 matching blocks also
        // read - consecutive memory whatever order the host's commPattern lists them in
        std::vector<int> db, hb;
        std::vector<long> dof, hof;
        if (make_list_host(level, cp.h_donorBlock.data(), cp.h_donorIdx.data(), nc, 0, nc, db, dof)) return 1;
        if (make_list_host(level, cp.h_haloBlock.data(), cp.h_haloIdx.data(), nc, 0, nc, hb, hof)) return 1;
        std::vector<int> perm(nc);
        for (int t = 0; t < nc; ++t) perm[t] = t;
        std::sort(perm.begin(), perm.end(), [&](int a, int c) { return hb[a] != hb[c] ? hb[a] < hb[c] : hof[a] < hof[c]; });
        std::vector<int> db2(nc), hb2(nc);
        std::vector<long> dof2(nc), hof2(nc);
        for (int t = 0; t < nc; ++t) { db2[t] = db[perm[t]]; dof2[t] = dof[perm[t]]; hb2[t] = hb[perm[t]]; hof2[t] = hof[perm[t]]; }
        if (g_comm_self && nc > 0) {
            // tuning "comm_self": the same-process interfaces take the inter-GPU path -- k_halo_pack, ncclSend / ncclRecv to the own
            // rank inside the group, k_halo_unpack -- so that the RCCL leg of whalo1 / whalo2 executes on a single GPU
            // (the t-th packed donor is the t-th unpacked halo)
            cp.local.n = 0;
            CommList s, r;
            s.n = r.n = nc;
            s.peer = r.peer = g_self_rank;
            if (upload_list(db2, dof2, &s.blkA, &s.offA)) return 1;
            if (upload_list(hb2, hof2, &r.blkA, &r.offA)) return 1;
            HIPCHK(hipMalloc((void**)&s.buf, sizeof(double) * 11 * (size_t)nc));
            HIPCHK(hipMalloc((void**)&r.buf, sizeof(double) * 11 * (size_t)nc));
            cp.sends.push_back(s);
            cp.recvs.push_back(r);
        } else {
            if (upload_list(db2, dof2, &cp.local.blkA, &cp.local.offA)) return 1;
            if (upload_list(hb2, hof2, &cp.local.blkB, &cp.local.offB)) return 1;
        }
    }
    const int ns = (int)cp.h_sendProc.size(), nr = (int)cp.h_recvProc.size();
    const int nst = ns ? cp.h_nsendCum[ns] : 0, nrt = nr ? cp.h_nrecvCum[nr] : 0;
    const int s0 = (int)cp.sends.size(), r0 = (int)cp.recvs.size();       // the self message, when there is one
    cp.sends.resize(s0 + ns);
    cp.recvs.resize(r0 + nr);
    for (int i = 0; i < ns; ++i) {
        CommList& l = cp.sends[s0 + i];
        l.peer = cp.h_sendProc[i];
        l.n = cp.h_nsendCum[i + 1] - cp.h_nsendCum[i];
        if (make_list(level, cp.h_sendBlock.data(), cp.h_sendIdx.data(), nst, cp.h_nsendCum[i], l.n, &l.blkA, &l.offA)) return 1;
        HIPCHK(hipMalloc((void**)&l.buf, sizeof(double) * 11 * (size_t)std::max(l.n, 1)));
    }
    for (int i = 0; i < nr; ++i) {
        CommList& l = cp.recvs[r0 + i];
        l.peer = cp.h_recvProc[i];
        l.n = cp.h_nrecvCum[i + 1] - cp.h_nrecvCum[i];
        if (make_list(level, cp.h_recvBlock.data(), cp.h_recvIdx.data(), nrt, cp.h_nrecvCum[i], l.n, &l.blkA, &l.offA)) return 1;
        HIPCHK(hipMalloc((void**)&l.buf, sizeof(double) * 11 * (size_t)std::max(l.n, 1)));
    }
    for (auto& pd : cp.periodic) {
        free_list(pd.list);
        pd.list.n = (int)pd.h_block.size();
        if (pd.list.n > 0 && make_list(level, pd.h_block.data(), pd.h_idx.data(), pd.list.n, 0, pd.list.n, &pd.list.blkA, &pd.list.offA))
            return 1;
    }
    cp.built = true;
    return 0;
}

// setCommPointers (haloExchange.F90:392-415): which variables travel
int halo_mask(int varStart, int varEnd, int commPressure, int commVisc, unsigned* mask, int* nvar)
{
    if (varStart < 1 || varEnd > 6) return fail("halo exchange: variable range %d..%d outside 1..6", varStart, varEnd);
    unsigned m = 0;
    int n = 0;
    for (int l = varStart; l <= varEnd; ++l) { m |= 1u << (l - 1); ++n; }
    if (commPressure) { m |= 1u << 8; ++n; }
    const bool visc = (g_opts.equations == ADFLOW_NS || g_opts.equations == ADFLOW_RANS);
    if (visc && commVisc) { m |= 1u << 9; ++n; }
    if (g_opts.equations == ADFLOW_RANS && commVisc) { m |= 1u << 10; ++n; }
    *mask = m;
    *nvar = n;
    return 0;
}

}  // namespace

#ifndef ADFLOW_NO_RCCL
#include <rccl/rccl.h>
namespace {
ncclComm_t g_nccl = nullptr;
int g_rank = 0, g_nranks = 1;
}
#define NCCLCHK(expr)                                                                          \
    do {                                                                                       \
        ncclResult_t r_ = (expr);                                                              \
        if (r_ != ncclSuccess) return fail("%s failed: %s", #expr, ncclGetErrorString(r_));    \
    } while (0)
#endif

extern "C" {

int adflow_gpu_set_bc_callback(adflow_bc_callback fn)
{
    ++g_state_gen;
    g_bc_callback = fn;
    return 0;
}

int adflow_gpu_bc_register(int nn, int level, int sps, int nBocos, int nViscBocos, const adflow_bc_subface* faces)
{
    ++g_state_gen;
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (nBocos < 0 || nViscBocos < 0 || nViscBocos > nBocos) return fail("bc_register: nBocos=%d nViscBocos=%d", nBocos, nViscBocos);
    if (nBocos > 0 && !faces) return fail("bc_register: null subface list");
    const BlkView& v = b->v;
    std::vector<BcFaceDev> out;
    std::vector<void*> fresh;       // device arrays of this registration
    auto drop_fresh = [&]() { for (void* q : fresh) (void)hipFree(q); };
    for (int m = 0; m < nBocos; ++m) {
        const adflow_bc_subface& f = faces[m];
        switch (f.bcType) {
        case ADFLOW_BC_SYMM: case ADFLOW_BC_NSWALL_ADIABATIC: case ADFLOW_BC_NSWALL_ISOTHERMAL: case ADFLOW_BC_EULERWALL:
        case ADFLOW_BC_FARFIELD: case ADFLOW_BC_SUPERSONIC_INFLOW: case ADFLOW_BC_SUPERSONIC_OUTFLOW: case ADFLOW_BC_EXTRAP:
        case ADFLOW_BC_SYMM_POLAR: case ADFLOW_BC_SUBSONIC_INFLOW: case ADFLOW_BC_SUBSONIC_OUTFLOW: case ADFLOW_BC_MASSBLEED_OUTFLOW:
            break;
        default:
            return drop_fresh(), fail("bc_register: block %d subface %d: BCType %d is not implemented on the device "
                        "(inflow bleeds, mDot / thrust, domain and sliding interfaces stay with the host callback)", nn, m + 1, f.bcType);
        }
        if (f.faceID < ADFLOW_IMIN || f.faceID > ADFLOW_KMAX) return drop_fresh(), fail("bc_register: block %d subface %d: BCFaceID %d", nn, m + 1, f.faceID);
        // generic subface indices run over the two in-plane directions of the block face (utils.F90:881-1175)
        const int amax = (f.faceID <= ADFLOW_IMAX) ? v.jb : v.ib;
        const int bmax = (f.faceID <= ADFLOW_JMAX) ? v.kb : v.jb;
        if (f.icBeg < 0 || f.icEnd > amax || f.jcBeg < 0 || f.jcEnd > bmax || f.icEnd < f.icBeg || f.jcEnd < f.jcBeg)
            return drop_fresh(), fail("bc_register: block %d subface %d: cell range %d:%d x %d:%d outside the block face", nn, m + 1, f.icBeg,
                        f.icEnd, f.jcBeg, f.jcEnd);
        const bool subOut = (f.bcType == ADFLOW_BC_SUBSONIC_OUTFLOW || f.bcType == ADFLOW_BC_MASSBLEED_OUTFLOW);
        const bool subIn = (f.bcType == ADFLOW_BC_SUBSONIC_INFLOW);
        const bool needNorm = (f.bcType == ADFLOW_BC_SYMM || f.bcType == ADFLOW_BC_EULERWALL || f.bcType == ADFLOW_BC_FARFIELD || subOut || subIn);
        if (subOut && !f.ps) return drop_fresh(), fail("bc_register: block %d subface %d: BCData%%ps is required", nn, m + 1);
        if (subIn) {
            if (f.subsonicInletTreatment == ADFLOW_INLET_TOTAL_CONDITIONS) {
                if (!(f.ptInlet && f.ttInlet && f.htInlet && f.flowXdirInlet && f.flowYdirInlet && f.flowZdirInlet))
                    return drop_fresh(), fail("bc_register: block %d subface %d: ptInlet, ttInlet, htInlet, flow[XYZ]dirInlet are required", nn, m + 1);
            } else if (f.subsonicInletTreatment == ADFLOW_INLET_MASS_FLOW) {
                if (!(f.rho && f.velx && f.vely && f.velz)) return drop_fresh(), fail("bc_register: block %d subface %d: rho, velx, vely, velz are required", nn, m + 1);
            } else
                return drop_fresh(), fail("bc_register: block %d subface %d: subsonicInletTreatment=%d (1 total conditions, 2 mass flow)", nn, m + 1,
                            f.subsonicInletTreatment);
        }
        if (f.bcType == ADFLOW_BC_SYMM_POLAR && !v.x) return drop_fresh(), fail("bc_register: block %d subface %d: symmPolar needs the node coordinates x", nn, m + 1);
        if ((subIn || f.bcType == ADFLOW_BC_SUPERSONIC_INFLOW) && v.nw > 5 && !f.turbInlet)
            return drop_fresh(), fail("bc_register: block %d subface %d: BCData%%turbInlet is required for an inflow subface of a RANS block", nn, m + 1);
        if (needNorm && !f.norm) return drop_fresh(), fail("bc_register: block %d subface %d: BCData%%norm is required", nn, m + 1);
        if (f.bcType == ADFLOW_BC_NSWALL_ISOTHERMAL && !f.TNS_Wall) return drop_fresh(), fail("bc_register: block %d subface %d: TNS_Wall is required", nn, m + 1);
        if (f.bcType == ADFLOW_BC_SUPERSONIC_INFLOW && !(f.rho && f.velx && f.vely && f.velz && f.ps))
            return drop_fresh(), fail("bc_register: block %d subface %d: rho, velx, vely, velz, ps are required", nn, m + 1);
        const size_t n = (size_t)(f.icEnd - f.icBeg + 1) * (f.jcEnd - f.jcBeg + 1);
        auto up = [&](const double* h, int nc, const double** dev) -> int {
            *dev = nullptr;
            if (!h) return 0;
            void* raw = nullptr;
            HIPCHK(hipMalloc(&raw, sizeof(double) * n * nc));
            HIPCHK(hipMemcpy(raw, h, sizeof(double) * n * nc, hipMemcpyHostToDevice));
            fresh.push_back(raw);
            *dev = (const double*)raw;
            return 0;
        };
        BcFaceDev d;
        d.type = f.bcType; d.faceID = f.faceID; d.icBeg = f.icBeg; d.icEnd = f.icEnd; d.jcBeg = f.jcBeg; d.jcEnd = f.jcEnd;
        if (up(f.norm, 3, &d.norm) || up(f.rface, 1, &d.rface) || up(f.uSlip, 3, &d.uslip) || up(f.TNS_Wall, 1, &d.tns) ||
            up(f.rho, 1, &d.rho) || up(f.velx, 1, &d.vx) || up(f.vely, 1, &d.vy) || up(f.velz, 1, &d.vz) || up(f.ps, 1, &d.ps) ||
            up(f.ptInlet, 1, &d.pt) || up(f.ttInlet, 1, &d.tt) || up(f.htInlet, 1, &d.ht) || up(f.flowXdirInlet, 1, &d.fdx) ||
            up(f.flowYdirInlet, 1, &d.fdy) || up(f.flowZdirInlet, 1, &d.fdz) || up(v.nw > 5 ? f.turbInlet : nullptr, 1, &d.turbInlet))
            return 1;
        d.inletTreatment = f.subsonicInletTreatment; d.pad = 0;
        for (int q = 0; q < 3; ++q) d.symNorm[q] = f.symNorm[q];
        d.tauq = nullptr;
        if (m < nViscBocos) {
            int r[4];
            bc_owned_range(f.faceID, f.icBeg, f.icEnd, f.jcBeg, f.jcEnd, v.il, v.jl, v.kl, r);
            const long no = (long)std::max(0, r[1] - r[0] + 1) * std::max(0, r[3] - r[2] + 1);
            if (no > 0) {
                void* raw = nullptr;
                HIPCHK(hipMalloc(&raw, sizeof(double) * 9 * no));
                HIPCHK(hipMemsetAsync(raw, 0, sizeof(double) * 9 * no, g_stream));
                fresh.push_back(raw);
                d.tauq = (double*)raw;
            }
        }
        out.push_back(d);
    }
    // the previous registration's device data is no longer referenced once the plan is dropped
    bc_plan_drop(level);
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    for (void* q : b->bc_allocs) (void)hipFree(q);
    b->bc_allocs = fresh;
    b->bc = out;
    b->nViscBocos = nViscBocos;
    b->tau_stored = false;
    for (void* q : b->fam_allocs) (void)hipFree(q);      // the families and the blanking belong to the subfaces they were set for
    b->fam_allocs.clear();
    b->famID.clear();
    b->faceBlank.clear();
    if (v.nw > 5 && !v.bmt[0]) {
        // face arrays of the implicit turbulence boundary treatment (bmt/bvt of blockPointers, one turbulence variable)
        const size_t nf[3] = {(size_t)v.je * v.ke, (size_t)v.ie * v.ke, (size_t)v.ie * v.je};
        for (int f6 = 0; f6 < 6; ++f6)
            for (int which = 0; which < 2; ++which) {
                void* raw = nullptr;
                HIPCHK(hipMalloc(&raw, sizeof(double) * nf[f6 / 2]));
                HIPCHK(hipMemsetAsync(raw, 0, sizeof(double) * nf[f6 / 2], g_stream));
                b->allocs.push_back(raw);
                (which ? b->v.bvt : b->v.bmt)[f6] = (double*)raw;
            }
        invalidate_comm_level(level);   // the device block table holds copies of BlkView
    } else if (v.nw > 5) {
        // a new registration: the faces that carry no subface any more must read bmt = bvt = 0 (the merged turbulence treatment
        // writes the cells of the subfaces only)
        const size_t nf[3] = {(size_t)v.je * v.ke, (size_t)v.ie * v.ke, (size_t)v.ie * v.je};
        for (int f6 = 0; f6 < 6; ++f6) {
            HIPCHK(hipMemsetAsync(b->v.bmt[f6], 0, sizeof(double) * nf[f6 / 2], g_stream));
            HIPCHK(hipMemsetAsync(b->v.bvt[f6], 0, sizeof(double) * nf[f6 / 2], g_stream));
        }
    }
    return 0;
}

// ---- launch plan of the boundary subfaces of a level (kernels_bc.hip): every subface of every block in one device
// array; `flow` lists the launches of applyAllBC in the reference's order, `ordinal` the r-th subfaces of all blocks
struct BcPlan {
    BcEntry* d_ent = nullptr;
    int* d_order = nullptr;
    std::vector<BcPhase> flow, ordinal;
    BcPhase wall = {0, 0, 0, 0};   // the viscous subfaces (wall stress storage), any order
    long maxFace = 0;
    bool anyEulerWall = false;
    int nent = 0;
};
static std::map<int, BcPlan> g_bcplan;

static void bc_plan_drop(int level)
{
    auto it = g_bcplan.find(level);
    if (it == g_bcplan.end()) return;
    if (it->second.d_ent) (void)hipFree(it->second.d_ent);
    if (it->second.d_order) (void)hipFree(it->second.d_order);
    g_bcplan.erase(it);
    (void)wi_drop(level);           // its table of wall subfaces points into the subfaces of the plan
}

static void bc_plan_drop_all()
{
    std::vector<int> levels;
    for (auto& kv : g_bcplan) levels.push_back(kv.first);
    for (int l : levels) bc_plan_drop(l);
}

static int bc_plan(int level, BcPlan** out)
{
    auto it = g_bcplan.find(level);
    if (it != g_bcplan.end()) { *out = &it->second; return 0; }
    BcPlan pl;
    std::vector<BcEntry> ent;
    struct Ref { int first, n, nVisc; };      // entries of one block: ent[first .. first+n)
    std::vector<Ref> blocks;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level || std::get<1>(kv.first) != 1) continue;
        Block* b = kv.second;
        if (b->bc.empty()) continue;
        Ref r = {(int)ent.size(), (int)b->bc.size(), b->nViscBocos};
        for (auto& f : b->bc) {
            BcEntry e;
            e.slot = std::get<2>(kv.first); e.pad = 0; e.f = f;
            ent.push_back(e);
            pl.anyEulerWall = pl.anyEulerWall || f.type == ADFLOW_BC_EULERWALL;
        }
        blocks.push_back(r);
        const BlkView& v = b->v;
        pl.maxFace = std::max(pl.maxFace, std::max(std::max((long)v.je * v.ke, (long)v.ie * v.ke), (long)v.ie * v.je));
    }
    pl.nent = (int)ent.size();
    std::vector<int> order;
    auto cells = [&](int e) { const BcFaceDev& f = ent[e].f; return (long)(f.icEnd - f.icBeg + 1) * (f.jcEnd - f.jcBeg + 1); };
    // kinds in the order of applyAllBC_block (BCRoutines.F90:75-216); walls only among the first nViscBocos subfaces
    auto match = [&](int kind, const BcFaceDev& f, bool inVisc) {
        switch (kind) {
        case BCP_SYMM1: case BCP_SYMM2: return f.type == ADFLOW_BC_SYMM;
        case BCP_WALL_ADIABATIC: return inVisc && f.type == ADFLOW_BC_NSWALL_ADIABATIC;
        case BCP_WALL_ISOTHERMAL: return inVisc && f.type == ADFLOW_BC_NSWALL_ISOTHERMAL;
        case BCP_FARFIELD: return f.type == ADFLOW_BC_FARFIELD;
        case BCP_EXTRAP: return f.type == ADFLOW_BC_EXTRAP || f.type == ADFLOW_BC_SUPERSONIC_OUTFLOW;
        case BCP_EULERWALL: return f.type == ADFLOW_BC_EULERWALL;
        case BCP_SUPERSONIC_INFLOW: return f.type == ADFLOW_BC_SUPERSONIC_INFLOW;
        case BCP_SYMMPOLAR1: case BCP_SYMMPOLAR2: return f.type == ADFLOW_BC_SYMM_POLAR;
        case BCP_SUBSONIC_OUTFLOW: return f.type == ADFLOW_BC_SUBSONIC_OUTFLOW || f.type == ADFLOW_BC_MASSBLEED_OUTFLOW;
        case BCP_SUBSONIC_INFLOW: return f.type == ADFLOW_BC_SUBSONIC_INFLOW;
        default: return true;
        }
    };
    auto add_kind = [&](int kind, std::vector<BcPhase>& dst) {
        for (int r = 0;; ++r) {       // r-th matching subface of every block: never two subfaces of one block together
            BcPhase ph = {kind, (int)order.size(), 0, 0};
            for (auto& rb : blocks) {
                int seen = 0;
                for (int m = 0; m < rb.n; ++m)
                    if (match(kind, ent[rb.first + m].f, m < rb.nVisc)) {
                        if (seen == r) { order.push_back(rb.first + m); ph.count++; ph.maxCells = std::max(ph.maxCells, cells(rb.first + m)); break; }
                        ++seen;
                    }
            }
            if (ph.count == 0) break;
            dst.push_back(ph);
        }
    };
    for (int kind : {BCP_SYMM1, BCP_SYMM2, BCP_SYMMPOLAR1, BCP_SYMMPOLAR2, BCP_WALL_ADIABATIC, BCP_WALL_ISOTHERMAL, BCP_FARFIELD,
                     BCP_SUBSONIC_OUTFLOW, BCP_SUBSONIC_INFLOW, BCP_EXTRAP, BCP_EULERWALL, BCP_SUPERSONIC_INFLOW})
        add_kind(kind, pl.flow);
    add_kind(BCP_ORDINAL, pl.ordinal);
    pl.wall.first = (int)order.size();
    for (int e = 0; e < (int)ent.size(); ++e)
        if (ent[e].f.tauq) {
            order.push_back(e);
            pl.wall.count++;
            // (the launch over the wall faces also covers the (n1 + 1) (n2 + 1) nodes of their plane: k_wall_node_grad)
            const BcFaceDev& f = ent[e].f;
            pl.wall.maxCells = std::max(pl.wall.maxCells, (long)(f.icEnd - f.icBeg + 2) * (f.jcEnd - f.jcBeg + 2));
        }
    if (pl.nent > 0) {
        HIPCHK(hipMalloc((void**)&pl.d_ent, sizeof(BcEntry) * ent.size()));
        HIPCHK(hipMemcpy(pl.d_ent, ent.data(), sizeof(BcEntry) * ent.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc((void**)&pl.d_order, sizeof(int) * order.size()));
        HIPCHK(hipMemcpy(pl.d_order, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice));
    }
    g_bcplan[level] = pl;
    *out = &g_bcplan[level];
    return 0;
}

// bcTurbTreatment of every block of the level with registered subfaces
static int turb_bc_treatment_enqueue(int level, const KParams& kp)
{
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (pl->nent == 0) return 0;
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_turb_bc_treatment(t.tab, t.n, pl->maxFace, pl->d_ent, pl->d_order, pl->ordinal, kp, g_stream);
    return 0;
}

// applyAllTurbBCThisBlock(secondHalo) of every block of the level
static int turb_bc_apply_enqueue(int level, const KParams& kp, int secondHalo)
{
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (pl->nent == 0) return 0;
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_apply_turb_bc(t.tab, pl->d_ent, pl->d_order, pl->ordinal, kp, secondHalo, g_stream);
    return 0;
}

// bcTurbTreatment + applyAllTurbBCThisBlock(secondHalo) for the blocks of `level` with registered subfaces
static int apply_turb_bc_enqueue(int level, int secondHalo)
{
    if (g_opts.equations != ADFLOW_RANS) return 0;
    KParams kp = make_kparams(level, 1.0, 0);
    if (turb_bc_treatment_enqueue(level, kp)) return 1;
    return turb_bc_apply_enqueue(level, kp, secondHalo);
}

// both, in the order of blocketteRes (blockette.F90:228-244): turbulence first
static int apply_turb_and_flow_bc_enqueue(int level, int secondHalo, bool turbBC)
{
    if (turbBC && apply_turb_bc_enqueue(level, secondHalo)) return 1;
    return apply_bc_enqueue(level, secondHalo);
}

// applyAllBC (BCRoutines.F90:15-54) for the blocks of `level` that registered subfaces
static int apply_bc_enqueue(int level, int secondHalo)
{
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (pl->nent == 0) return 0;
    KParams kp = make_kparams(level, 1.0, 0);
    if (pl->anyEulerWall && g_opts.eulerWallBCTreatment == ADFLOW_WALLBC_QUADRATIC)
        return fail("eulerWallBCTreatment=%d: bcEulerWall has no quadratic extrapolation (1 constant, 2 linear, 4 normal momentum)",
                    g_opts.eulerWallBCTreatment);
    if (pl->anyEulerWall && g_opts.eulerWallBCTreatment == ADFLOW_WALLBC_NORMAL_MOMENTUM && kp.fineGrid) {
        if (!level_at_rest(level))
            return fail("eulerWallBCTreatment = normal momentum on moving blocks needs the cell-centre grid velocity (not mirrored)");
    }
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_apply_all_bc(t.tab, pl->d_ent, pl->d_order, pl->flow, kp, secondHalo, g_opts.eulerWallBCTreatment,
                        g_opts.viscWallBCTreatment, g_opts.outflowTreatment, g_opts.hScalingInlet, g_stream);
    return for_level(level, [&](Block* b) {
        if (!b->bc.empty()) b->ss_valid = false;
        return 0;
    });
}

// bcTurbTreatment_d + applyAllTurbBCThisBlock_d + applyAllBC_block_d on the dual arrays of the level (kernels_ad.hip)
static int ad_apply_bc_enqueue(int level, const KParams& kp, bool turbBC)
{
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (pl->nent == 0) return 0;
    if (pl->anyEulerWall && g_opts.eulerWallBCTreatment == ADFLOW_WALLBC_QUADRATIC)
        return fail("eulerWallBCTreatment=%d: bcEulerWall has no quadratic extrapolation", g_opts.eulerWallBCTreatment);
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    if (turbBC) ad_launch_turb_bc(g_ad_tab, t.n, pl->maxFace, pl->d_ent, pl->d_order, pl->ordinal, kp, 1, g_stream);
    // applyAllBC_block_d (src/adjoint/outputForward/BCExtra_d.F90:10-139) applies the kinds that were differentiated: symmetry,
    // polar symmetry, viscous walls, farfield, subsonic out- / inflow, Euler wall.  Extrapolation and the supersonic kinds are NOT
    // in it: their halos keep the values of the last primal boundary-condition pass with a zero derivative.  Reproduced.
    std::vector<BcPhase> flow;
    for (const BcPhase& ph : pl->flow)
        if (ph.kind != BCP_EXTRAP && ph.kind != BCP_SUPERSONIC_INFLOW) flow.push_back(ph);
    ad_launch_apply_all_bc(g_ad_tab, pl->d_ent, pl->d_order, flow, kp, 1, g_opts.eulerWallBCTreatment, g_opts.viscWallBCTreatment,
                           g_opts.outflowTreatment, g_opts.hScalingInlet, g_stream);
    return 0;
}

static bool has_wall_subfaces(int level)
{
    BcPlan* pl;
    if (bc_plan(level, &pl)) return false;
    return pl->wall.count > 0;
}

// viscSubface(:)%tau / %q of every viscous subface of the level, from the nodal gradients the viscous kernels just used
static int wall_stress_enqueue(int level, const KParams& kp, bool formGrad)
{
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (pl->wall.count == 0) return 0;
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_wall_stress(t.tab, pl->d_ent, pl->d_order, pl->wall, kp, formGrad, g_stream);
    return for_level(level, [&](Block* b) {
        if (b->nViscBocos > 0) b->tau_stored = true;
        return 0;
    });
}

int adflow_gpu_download_wall_stress(int nn, int level, int sps, int mm, double* tau, double* q)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (mm < 1 || mm > b->nViscBocos || mm > (int)b->bc.size()) return fail("download_wall_stress: subface %d is not a viscous subface of block %d", mm, nn);
    const BcFaceDev& f = b->bc[mm - 1];
    int r[4];
    bc_owned_range(f.faceID, f.icBeg, f.icEnd, f.jcBeg, f.jcEnd, b->v.il, b->v.jl, b->v.kl, r);
    const long no = (long)std::max(0, r[1] - r[0] + 1) * std::max(0, r[3] - r[2] + 1);
    if (no == 0 || !f.tauq) return 0;
    HIPCHK(hipStreamSynchronize(g_stream));
    if (tau) HIPCHK(hipMemcpy(tau, f.tauq, sizeof(double) * 6 * no, hipMemcpyDeviceToHost));
    if (q) HIPCHK(hipMemcpy(q, f.tauq + 6 * no, sizeof(double) * 3 * no, hipMemcpyDeviceToHost));
    return 0;
}

// ---- surface integration (kernels_wallint.hip): wallIntegrationFace over the wall subfaces of a level -------------------------------
static bool is_wall_type(int t) { return t == ADFLOW_BC_EULERWALL || t == ADFLOW_BC_NSWALL_ADIABATIC || t == ADFLOW_BC_NSWALL_ISOTHERMAL; }

// What the first integration of a level allocates: the table of wall subfaces, 7 doubles per owned wall face, the partial results of
// the face kernel, the membership table of the groups and the output of the host form.  Dropped with the boundary plan of the level
// and by adflow_gpu_release_workspace.
struct WiLevel {
    struct Ref { int nn, mm, fam; long no; double* fpv; };      // block, subface (1-based), family, owned faces, its per-face buffer
    std::vector<Ref> faces;
    WiFace* d_faces = nullptr;
    long maxOwned = 0;
    double* part = nullptr;
    unsigned char* d_member = nullptr;
    std::vector<unsigned char> member;      // host copy of the table on the device: a call with the same groups uploads nothing
    int memberGroups = 0;
    double* d_out = nullptr;                // the host form's output, memberGroups x ADFLOW_WALLINT_STRIDE
    bool integrated = false;
    // the derivative entries (adflow_gpu_wall_integrate_fwd / _bwd), allocated by the first call that needs them
    long nOwned = 0, maxBox = 0;            // owned wall faces of the level; the most cells of a subface's box (k_wallint_credit)
    void* partD = nullptr;                  // the partial results of the dual face kernel
    double* d_dot = nullptr;                // the host form's out and outDot, 2 x dotGroups x ADFLOW_WALLINT_STRIDE
    int dotGroups = 0;
    int barNS = 0, barNv = 0;               // what the buffers of the transposed product were laid out for
    std::vector<void*> barAllocs;
    std::vector<double> wq;                 // host copy of the weights on the device
    double *d_wq = nullptr, *d_g = nullptr; // weights per (set, subface, quantity); contracted derivatives per (set, owned face)
    JmBlk* barTab = nullptr;                // per weight set the level's table with ys = the halo'd result
    std::vector<double*> barYs;             // per block slot its ys of all sets (with the front padding)
    std::vector<size_t> barYsBytes;
    int64_t barBytes = 0;                   // of barAllocs, part of bytes
    int barSlots = 0, barNx = 0, barNy = 0, barNz = 0;
    int nq = WI_NQ;                         // quantities per workgroup of the face kernel (FI_NQ in the record of the flow subfaces)
    std::vector<void*> allocs;
    int64_t bytes = 0;
};
static std::map<int, WiLevel> g_wi;
static std::map<int, WiLevel> g_fi;      // the same record for the in- and outflow subfaces (adflow_gpu_flow_integrate): same lifetime

static int64_t wi_drop_in(std::map<int, WiLevel>& recs, int level)
{
    auto it = recs.find(level);
    if (it == recs.end()) return 0;
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    for (void* p : it->second.allocs) (void)hipFree(p);
    for (void* p : it->second.barAllocs) (void)hipFree(p);
    const int64_t n = it->second.bytes;
    recs.erase(it);
    return n;
}

static int64_t wi_drop(int level) { return wi_drop_in(g_wi, level) + wi_drop_in(g_fi, level); }

static int64_t wi_drop_all()
{
    std::vector<int> levels;
    for (auto& kv : g_wi) levels.push_back(kv.first);
    for (auto& kv : g_fi) levels.push_back(kv.first);
    int64_t n = 0;
    for (int l : levels) n += wi_drop(l);
    return n;
}

static int wi_alloc(WiLevel& L, void** p, size_t bytes)
{
    HIPCHK(hipMalloc(p, bytes));
    L.allocs.push_back(*p);
    L.bytes += (int64_t)bytes;
    return 0;
}

// the table of wall subfaces of the level and their buffers (the order of g_blocks: block, then subface)
static int wi_build(int level, WiLevel& L)
{
    std::vector<WiFace> tab;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level || std::get<1>(kv.first) != 1) continue;
        Block* b = kv.second;
        for (int m = 0; m < (int)b->bc.size(); ++m) {
            const BcFaceDev& f = b->bc[m];
            if (!is_wall_type(f.type)) continue;
            WiFace w;
            w.slot = std::get<2>(kv.first); w.faceID = f.faceID;
            bc_owned_range(f.faceID, f.icBeg, f.icEnd, f.jcBeg, f.jcEnd, b->v.il, b->v.jl, b->v.kl, w.r);
            const long no = (long)std::max(0, w.r[1] - w.r[0] + 1) * std::max(0, w.r[3] - w.r[2] + 1);
            if (no == 0) continue;
            w.icBeg = f.icBeg; w.jcBeg = f.jcBeg; w.ldn = f.icEnd - f.icBeg + 1; w.inflow = 0;
            w.nnorm = (long)w.ldn * (f.jcEnd - f.jcBeg + 1);
            w.norm = f.norm;
            w.tauq = (m < b->nViscBocos && f.type != ADFLOW_BC_EULERWALL) ? f.tauq : nullptr;
            w.iblank = m < (int)b->faceBlank.size() ? b->faceBlank[m] : nullptr;
            void* raw = nullptr;
            if (wi_alloc(L, &raw, sizeof(double) * 7 * (size_t)no)) return 1;
            HIPCHK(hipMemsetAsync(raw, 0, sizeof(double) * 7 * (size_t)no, g_stream));
            w.fpv = (double*)raw;
            w.goff = L.nOwned;
            L.nOwned += no;
            L.maxBox = std::max(L.maxBox, (long)(w.r[1] - w.r[0] + 1 + 2 * WI_REACH) * (w.r[3] - w.r[2] + 1 + 2 * WI_REACH) * WI_DEPTH);
            tab.push_back(w);
            WiLevel::Ref r = {std::get<2>(kv.first), m + 1, m < (int)b->famID.size() ? b->famID[m] : 0, no, w.fpv};
            L.faces.push_back(r);
            L.maxOwned = std::max(L.maxOwned, no);
        }
    }
    if (tab.empty()) return 0;
    if (wi_alloc(L, (void**)&L.d_faces, sizeof(WiFace) * tab.size())) return 1;
    HIPCHK(hipMemcpy(L.d_faces, tab.data(), sizeof(WiFace) * tab.size(), hipMemcpyHostToDevice));
    const size_t nwg = (size_t)wallint_groups_per_face(L.maxOwned) * tab.size();
    return wi_alloc(L, (void**)&L.part, sizeof(double) * WI_NQ * nwg);
}

static int wi_check_groups(const char* who, int nGroups, const int32_t* famLists, int ldFam)
{
    if (nGroups < 0) return fail("%s: nGroups = %d", who, nGroups);
    if (nGroups > 0) {
        if (!famLists || ldFam < 1) return fail("%s: nGroups = %d needs famLists with ldFam >= 1 (ldFam = %d)", who, nGroups, ldFam);
        for (int g = 0; g < nGroups; ++g)
            if (famLists[g] < 0 || famLists[g] > ldFam - 1)
                return fail("%s: group %d lists %d families, famLists holds at most ldFam - 1 = %d", who, g + 1, famLists[g], ldFam - 1);
    }
    return 0;
}

// the membership table of the groups on the device, and the output of the host form; nG: the groups of the output (1 for nGroups = 0)
static int wi_members(WiLevel& L, int nGroups, const int32_t* famLists, int* nGout)
{
    const int nface = (int)L.faces.size();
    const int nG = nGroups > 0 ? nGroups : 1;
    // member[g nface + f]: famInList(BCData(mm)%famID, famLists(g, 2:1 + famLists(g, 1))) of integrateSurfaces
    std::vector<unsigned char> member((size_t)nG * std::max(nface, 1), 0);
    for (int g = 0; g < nG; ++g)
        for (int f = 0; f < nface; ++f) {
            bool in = nGroups == 0;
            for (int j = 1; !in && j <= famLists[g]; ++j) in = famLists[g + (size_t)nGroups * j] == L.faces[f].fam;
            member[(size_t)g * nface + f] = in;
        }
    if (member != L.member || !L.d_member) {
        // (the kernels of an earlier enqueue-only call may still read the table)
        HIPCHK(hipStreamSynchronize(g_stream));
        if (nG > L.memberGroups) {
            void* raw = nullptr;
            if (wi_alloc(L, &raw, member.size())) return 1;
            L.d_member = (unsigned char*)raw;
            if (wi_alloc(L, &raw, sizeof(double) * ADFLOW_WALLINT_STRIDE * (size_t)nG)) return 1;
            L.d_out = (double*)raw;
            L.memberGroups = nG;
            L.member.clear();
        }
        HIPCHK(hipMemcpy(L.d_member, member.data(), member.size(), hipMemcpyHostToDevice));
        L.member = member;
    }
    *nGout = nG;
    return 0;
}

// What every entry of the integration does before it launches: the checks of par and of the groups, the parameters of the face kernel,
// the level's record with its table of wall subfaces, and the membership table of the groups on the device.  needStress: the entry
// reads the stored wall stress (the derivative entries form the stress of their own pass).  nG: the groups of the output (1 for
// nGroups = 0)
static int wi_setup(const char* who, int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, bool needStress,
                    WiPar* Pout, WiLevel** Lout, int* nGout)
{
    if (need_ready()) return 1;
    if (!par) return fail("%s: par must not be NULL", who);
    if (wi_check_groups(who, nGroups, famLists, ldFam)) return 1;
    const double MachCoef = par[ADFLOW_WALLINT_MACHCOEF];
    if (!(MachCoef > 0.0)) return fail("%s: MachCoef = %g must be positive", who, MachCoef);
    WiPar P;
    P.pInf = g_opts.pInf; P.pRef = g_opts.pRef; P.gammaInf = g_opts.gammaInf; P.MachCoef = MachCoef;
    double axisLen = 0.0;
    for (int d = 0; d < 3; ++d) {
        P.refPoint[d] = g_opts.LRef * par[ADFLOW_WALLINT_POINTREF + d];
        P.axisPoint[d] = g_opts.LRef * par[ADFLOW_WALLINT_MOMENTAXIS + d];
        P.axisDir[d] = g_opts.LRef * par[ADFLOW_WALLINT_MOMENTAXIS + 3 + d] - P.axisPoint[d];
        axisLen += P.axisDir[d] * P.axisDir[d];
        P.velDir[d] = par[ADFLOW_WALLINT_VELDIRFREESTREAM + d];
    }
    axisLen = sqrt(axisLen);
    if (!(axisLen > 0.0)) return fail("%s: the moment axis (LRef momentAxis) has zero length", who);
    for (int d = 0; d < 3; ++d) P.axisDir[d] /= axisLen;
    P.sepOffset = par[ADFLOW_WALLINT_SEPSENSOROFFSET]; P.sepSharpness = par[ADFLOW_WALLINT_SEPSENSORSHARPNESS];
    P.computeCavitation = par[ADFLOW_WALLINT_COMPUTECAVITATION] != 0.0;
    P.cavitationNumber = par[ADFLOW_WALLINT_CAVITATIONNUMBER]; P.cavOffset = par[ADFLOW_WALLINT_CAVSENSOROFFSET];
    P.cavSharpness = par[ADFLOW_WALLINT_CAVSENSORSHARPNESS];
    const double ce = par[ADFLOW_WALLINT_CAVEXPONENT];
    if (P.computeCavitation && !(ce >= 0.0 && ce <= 64.0 && ce == (double)(int)ce))
        return fail("%s: cavExponent = %g must be a whole number in 0 .. 64", who, ce);
    P.cavExponent = P.computeCavitation ? (int)ce : 0;
    P.cpminRho = par[ADFLOW_WALLINT_CPMIN_RHO]; P.cpminFamily = par[ADFLOW_WALLINT_CPMIN_FAMILY];
    P.rans = g_opts.equations == ADFLOW_RANS; P.pad = 0;

    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (pl->nent == 0) return fail("%s: level %d has no registered boundary subfaces (adflow_gpu_bc_register)", who, level);
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level || std::get<1>(kv.first) != 1) continue;
        const Block* b = kv.second;
        for (int m = 0; m < (int)b->bc.size(); ++m) {
            const BcFaceDev& f = b->bc[m];
            if (!is_wall_type(f.type) || f.type == ADFLOW_BC_EULERWALL || m >= b->nViscBocos || !f.tauq) continue;
            if (needStress && !b->tau_stored)
                return fail("%s: the wall stress of viscous subface %d of block %d was never stored (no storing residual evaluation "
                            "since adflow_gpu_bc_register)", who, m + 1, std::get<2>(kv.first));
            if (P.rans && !f.norm)
                return fail("%s: viscous subface %d of block %d was registered without BCData%%norm, which y+ reads", who, m + 1,
                            std::get<2>(kv.first));
        }
    }
    if (ensure_table(level)) return 1;
    auto it = g_wi.find(level);
    if (it == g_wi.end()) {
        WiLevel fresh;
        if (wi_build(level, fresh)) {
            for (void* p : fresh.allocs) (void)hipFree(p);
            return 1;
        }
        if (fresh.faces.size() > 65535) {
            for (void* p : fresh.allocs) (void)hipFree(p);
            return fail("%s: %zu wall subfaces on level %d, one launch takes 65535", who, fresh.faces.size(), level);
        }
        it = g_wi.emplace(level, std::move(fresh)).first;
    }
    if (wi_members(it->second, nGroups, famLists, nGout)) return 1;
    *Pout = P; *Lout = &it->second;
    return 0;
}

static int wall_integrate(const char* who, int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out,
                          bool outOnDevice)
{
    if (need_ready()) return 1;
    if (!par || !out) return fail("%s: par and out must not be NULL", who);
    WiPar P;
    WiLevel* Lp;
    int nG;
    if (wi_setup(who, level, par, nGroups, famLists, ldFam, true, &P, &Lp, &nG)) return 1;
    WiLevel& L = *Lp;
    const int nface = (int)L.faces.size();
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    double* d_out = outOnDevice ? out : L.d_out;
    launch_wallint(t.tab, L.d_faces, nface, L.maxOwned, P, L.part, L.d_member, nG, d_out, g_stream);
    L.integrated = true;
    if (outOnDevice) return sync_and_check();
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * ADFLOW_WALLINT_STRIDE * (size_t)nG, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

int adflow_gpu_bc_set_families(int nn, int level, int sps, int nBocos, const int32_t* famID, const int8_t* const* iblank)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (nBocos != (int)b->bc.size()) return fail("bc_set_families: block %d has %d registered subfaces, not %d", nn, (int)b->bc.size(), nBocos);
    if (nBocos > 0 && !famID) return fail("bc_set_families: famID is NULL");
    std::vector<void*> fresh;
    std::vector<const signed char*> blank((size_t)nBocos, nullptr);
    for (int m = 0; m < nBocos; ++m) {
        if (!iblank || !iblank[m]) continue;
        const BcFaceDev& f = b->bc[m];
        int r[4];
        bc_owned_range(f.faceID, f.icBeg, f.icEnd, f.jcBeg, f.jcEnd, b->v.il, b->v.jl, b->v.kl, r);
        const long no = (long)std::max(0, r[1] - r[0] + 1) * std::max(0, r[3] - r[2] + 1);
        if (no == 0) continue;
        void* raw = nullptr;
        if (hipMalloc(&raw, (size_t)no) != hipSuccess || hipMemcpy(raw, iblank[m], (size_t)no, hipMemcpyHostToDevice) != hipSuccess) {
            if (raw) (void)hipFree(raw);
            for (void* q : fresh) (void)hipFree(q);
            return fail("bc_set_families: the blanking of subface %d of block %d could not be copied to the device", m + 1, nn);
        }
        fresh.push_back(raw);
        blank[m] = (const signed char*)raw;
    }
    (void)wi_drop(level);            // (waits for the queue) its table holds the old families and blanking arrays
    for (void* q : b->fam_allocs) (void)hipFree(q);
    b->fam_allocs = fresh;
    b->faceBlank = blank;
    b->famID.assign(famID, famID + nBocos);
    return 0;
}

int adflow_gpu_wall_integrate(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out)
{
    return wall_integrate("wall_integrate", level, par, nGroups, famLists, ldFam, out, false);
}

int adflow_gpu_wall_integrate_dev(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out)
{
    return wall_integrate("wall_integrate_dev", level, par, nGroups, famLists, ldFam, out, true);
}

int adflow_gpu_download_wall_forces(int nn, int level, int sps, int mm, double* Fp, double* Fv, double* area)
{
    Block* b = find_block(nn, level, sps);
    if (!b) return fail("block (%d,%d,%d) not registered", nn, level, sps);
    if (mm < 1 || mm > (int)b->bc.size() || !is_wall_type(b->bc[mm - 1].type))
        return fail("download_wall_forces: subface %d is not a wall subface of block %d", mm, nn);
    auto it = g_wi.find(level);
    if (it == g_wi.end() || !it->second.integrated)
        return fail("download_wall_forces: no integration of level %d to read (adflow_gpu_wall_integrate; adflow_gpu_release_workspace frees it)", level);
    for (const WiLevel::Ref& r : it->second.faces) {
        if (r.nn != nn || r.mm != mm) continue;
        HIPCHK(hipStreamSynchronize(g_stream));
        if (Fp) HIPCHK(hipMemcpy(Fp, r.fpv, sizeof(double) * 3 * r.no, hipMemcpyDeviceToHost));
        if (Fv) HIPCHK(hipMemcpy(Fv, r.fpv + 3 * r.no, sizeof(double) * 3 * r.no, hipMemcpyDeviceToHost));
        if (area) HIPCHK(hipMemcpy(area, r.fpv + 6 * r.no, sizeof(double) * r.no, hipMemcpyDeviceToHost));
        return 0;
    }
    return 0;        // a subface without owned face cells
}

// ---- flow integration (kernels_wallint.hip): flowIntegrationFace over the in- and outflow subfaces of a level -----------------------
static bool is_flow_type(int t)
{
    return t == ADFLOW_BC_SUBSONIC_INFLOW || t == ADFLOW_BC_SUPERSONIC_INFLOW || t == ADFLOW_BC_SUBSONIC_OUTFLOW ||
           t == ADFLOW_BC_SUPERSONIC_OUTFLOW;
}

// the table of in- and outflow subfaces of the level (the order of g_blocks: block, then subface) and the partial results
static int fi_build(int level, WiLevel& L)
{
    std::vector<WiFace> tab;
    L.nq = FI_NQ;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level || std::get<1>(kv.first) != 1) continue;
        Block* b = kv.second;
        for (int m = 0; m < (int)b->bc.size(); ++m) {
            const BcFaceDev& f = b->bc[m];
            if (!is_flow_type(f.type)) continue;
            WiFace w;
            memset(&w, 0, sizeof(w));
            w.slot = std::get<2>(kv.first); w.faceID = f.faceID;
            bc_owned_range(f.faceID, f.icBeg, f.icEnd, f.jcBeg, f.jcEnd, b->v.il, b->v.jl, b->v.kl, w.r);
            const long no = (long)std::max(0, w.r[1] - w.r[0] + 1) * std::max(0, w.r[3] - w.r[2] + 1);
            if (no == 0) continue;
            w.inflow = (f.type == ADFLOW_BC_SUBSONIC_INFLOW || f.type == ADFLOW_BC_SUPERSONIC_INFLOW) ? 1 : 0;
            w.iblank = m < (int)b->faceBlank.size() ? b->faceBlank[m] : nullptr;
            w.goff = L.nOwned;
            L.nOwned += no;
            L.maxBox = std::max(L.maxBox, (long)(w.r[1] - w.r[0] + 1 + 2 * WI_REACH) * (w.r[3] - w.r[2] + 1 + 2 * WI_REACH) * WI_DEPTH);
            tab.push_back(w);
            WiLevel::Ref r = {std::get<2>(kv.first), m + 1, m < (int)b->famID.size() ? b->famID[m] : 0, no, nullptr};
            L.faces.push_back(r);
            L.maxOwned = std::max(L.maxOwned, no);
        }
    }
    if (tab.empty()) return 0;
    if (tab.size() > 65535) return fail("%zu in- and outflow subfaces on level %d, one launch takes 65535", tab.size(), level);
    if (wi_alloc(L, (void**)&L.d_faces, sizeof(WiFace) * tab.size())) return 1;
    HIPCHK(hipMemcpy(L.d_faces, tab.data(), sizeof(WiFace) * tab.size(), hipMemcpyHostToDevice));
    const size_t nwg = (size_t)wallint_groups_per_face(L.maxOwned) * tab.size();
    return wi_alloc(L, (void**)&L.part, sizeof(double) * FI_NQ * nwg);
}

// wi_setup for the flow subfaces: the checks, the parameters, the level's record and the membership table
static int fi_setup(const char* who, int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, FiPar* Pout,
                    WiLevel** Lout, int* nGout)
{
    if (need_ready()) return 1;
    if (!par) return fail("%s: par must not be NULL", who);
    if (wi_check_groups(who, nGroups, famLists, ldFam)) return 1;
    FiPar P;
    P.pInf = g_opts.pInf; P.pRef = g_opts.pRef; P.gammaInf = g_opts.gammaInf; P.TRef = g_opts.TRef; P.uRef = g_opts.uRef;
    P.timeRef = g_opts.timeRef; P.RGas = g_opts.RGas;
    P.rhoRef = par[ADFLOW_FLOWINT_RHOREF]; P.rGasDim = par[ADFLOW_FLOWINT_RGASDIM];
    P.internalFlowFact = par[ADFLOW_FLOWINT_INTERNALFLOW] != 0.0 ? -1.0 : 1.0;
    for (int d = 0; d < 3; ++d) P.refPoint[d] = g_opts.LRef * par[ADFLOW_FLOWINT_POINTREF + d];
    if (!(P.rhoRef > 0.0) || !(P.rGasDim > 0.0)) return fail("%s: rhoRef = %g and rGasDim = %g must be positive", who, P.rhoRef, P.rGasDim);
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (pl->nent == 0) return fail("%s: level %d has no registered boundary subfaces (adflow_gpu_bc_register)", who, level);
    if (ensure_table(level)) return 1;
    auto it = g_fi.find(level);
    if (it == g_fi.end()) {
        WiLevel fresh;
        if (fi_build(level, fresh)) {
            for (void* p : fresh.allocs) (void)hipFree(p);
            return 1;
        }
        it = g_fi.emplace(level, std::move(fresh)).first;
    }
    if (wi_members(it->second, nGroups, famLists, nGout)) return 1;
    *Pout = P; *Lout = &it->second;
    return 0;
}

static int flow_integrate(const char* who, int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out,
                          bool outOnDevice)
{
    if (need_ready()) return 1;
    if (!par || !out) return fail("%s: par and out must not be NULL", who);
    FiPar P;
    WiLevel* Lp;
    int nG;
    if (fi_setup(who, level, par, nGroups, famLists, ldFam, &P, &Lp, &nG)) return 1;
    WiLevel& L = *Lp;
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    double* d_out = outOnDevice ? out : L.d_out;
    launch_flowint(t.tab, L.d_faces, (int)L.faces.size(), L.maxOwned, P, L.part, L.d_member, nG, d_out, g_stream);
    if (outOnDevice) return sync_and_check();
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * ADFLOW_WALLINT_STRIDE * (size_t)nG, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

int adflow_gpu_flow_integrate(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out)
{
    return flow_integrate("flow_integrate", level, par, nGroups, famLists, ldFam, out, false);
}

int adflow_gpu_flow_integrate_dev(int level, const double* par, int nGroups, const int32_t* famLists, int ldFam, double* out)
{
    return flow_integrate("flow_integrate_dev", level, par, nGroups, famLists, ldFam, out, true);
}

// setCorrectionsCoarseHalos of every coarse block with subfaces (multiGrid.F90:472)
static int bc_coarse_corrections_enqueue(int coarseLevel, double fact)
{
    BcPlan* pl;
    if (bc_plan(coarseLevel, &pl)) return 1;
    if (pl->nent == 0) return 0;
    LevelTab t;
    if (level_tab(coarseLevel, &t)) return 1;
    launch_bc_coarse_corrections(t.tab, pl->d_ent, pl->d_order, pl->ordinal, fact, g_stream);
    return 0;
}

int adflow_gpu_apply_all_bc(int level, int secondHalo)
{
    if (need_ready()) return 1;
    if (apply_bc_enqueue(level, secondHalo)) return 1;
    return sync_and_check();
}

int adflow_gpu_comm_unique_id(void* id128)
{
#ifndef ADFLOW_NO_RCCL
    if (!id128) return fail("null id buffer");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return 0;
#else
    (void)id128;
    return fail("built without RCCL");
#endif
}

int adflow_gpu_comm_init(int rank, int nranks, const void* id128)
{
#ifndef ADFLOW_NO_RCCL
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    if (!id128) return fail("null id buffer");
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    NCCLCHK(ncclCommInitRank(&g_nccl, nranks, id, rank));
    g_rank = rank;
    g_nranks = nranks;
    g_self_rank = rank;
    return 0;
#else
    (void)rank; (void)nranks; (void)id128;
    return fail("built without RCCL");
#endif
}

int adflow_gpu_comm_info(int* rank, int* nranks, int* commCount, int* commUserRank)
{
    int cnt = -1, ur = -1;
#ifndef ADFLOW_NO_RCCL
    if (rank) *rank = g_rank;
    if (nranks) *nranks = g_nranks;
    if (g_nccl) {
        NCCLCHK(ncclCommCount(g_nccl, &cnt));
        NCCLCHK(ncclCommUserRank(g_nccl, &ur));
    }
#else
    if (rank) *rank = 0;
    if (nranks) *nranks = 1;
#endif
    if (commCount) *commCount = cnt;
    if (commUserRank) *commUserRank = ur;
    return 0;
}

int adflow_gpu_comm_register(int level, int nLayers, const adflow_comm_pattern* p)
{
    ++g_state_gen;
    ++g_pc_topo_gen;
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    if (!p) return fail("null comm pattern");
    if (nLayers < 0 || nLayers > 2) return fail("nLayers must be 1 or 2 (cell halos) or 0 (the node pattern of exchangeCoor)");
    auto key = std::make_pair(level, nLayers);
    if (g_comm.count(key)) {
        drop_comm_lists(g_comm[key]);     // a re-registration also drops the periodic transformations
    }
    CommPattern cp;
    cp.present = true;
    const int nc = p->ncopy;
    if (nc < 0 || p->nProcSend < 0 || p->nProcRecv < 0) return fail("negative count in comm pattern");
    if (nc > 0) {
        cp.h_donorBlock.assign(p->donorBlock, p->donorBlock + nc);
        cp.h_haloBlock.assign(p->haloBlock, p->haloBlock + nc);
        cp.h_donorIdx.assign(p->donorIndices, p->donorIndices + 3 * (size_t)nc);
        cp.h_haloIdx.assign(p->haloIndices, p->haloIndices + 3 * (size_t)nc);
    }
    if (p->nProcSend > 0) {
        cp.h_sendProc.assign(p->sendProc, p->sendProc + p->nProcSend);
        cp.h_nsendCum.assign(p->nsendCum, p->nsendCum + p->nProcSend + 1);
        const int nt = cp.h_nsendCum[p->nProcSend];
        cp.h_sendBlock.assign(p->sendBlock, p->sendBlock + nt);
        cp.h_sendIdx.assign(p->sendIndices, p->sendIndices + 3 * (size_t)nt);
    }
    if (p->nProcRecv > 0) {
        cp.h_recvProc.assign(p->recvProc, p->recvProc + p->nProcRecv);
        cp.h_nrecvCum.assign(p->nrecvCum, p->nrecvCum + p->nProcRecv + 1);
        const int nt = cp.h_nrecvCum[p->nProcRecv];
        cp.h_recvBlock.assign(p->recvBlock, p->recvBlock + nt);
        cp.h_recvIdx.assign(p->recvIndices, p->recvIndices + 3 * (size_t)nt);
    }
    g_comm[key] = cp;
    return 0;
}

int adflow_gpu_comm_register_periodic(int level, int nLayers, int nPeriodic, const adflow_periodic_data* pd)
{
    ++g_state_gen;
    ++g_pc_topo_gen;
    auto it = g_comm.find(std::make_pair(level, nLayers));
    if (it == g_comm.end()) return fail("comm_register_periodic: no pattern registered for level %d, nLayers %d", level, nLayers);
    if (nPeriodic < 0 || (nPeriodic > 0 && !pd)) return fail("comm_register_periodic: nPeriodic=%d", nPeriodic);
    CommPattern& cp = it->second;
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    drop_comm_lists(cp);
    cp.periodic.clear();
    for (int m = 0; m < nPeriodic; ++m) {
        CommPattern::Periodic q;
        for (int a = 0; a < 9; ++a) q.rotMatrix[a] = pd[m].rotMatrix[a];
        for (int a = 0; a < 3; ++a) { q.rotCenter[a] = pd[m].rotCenter[a]; q.translation[a] = pd[m].translation[a]; }
        const int n = pd[m].nHalos;
        if (n < 0 || (n > 0 && (!pd[m].block || !pd[m].indices))) return fail("comm_register_periodic: entry %d: nHalos=%d", m + 1, n);
        q.h_block.assign(pd[m].block, pd[m].block + n);
        q.h_idx.assign(pd[m].indices, pd[m].indices + (size_t)3 * n);
        cp.periodic.push_back(q);
    }
    return 0;
}

int adflow_gpu_halo_local_copy(int level, int nLayers, int varStart, int varEnd, int commPressure, int commVisc)
{
    if (need_ready()) return 1;
    CommPattern* cp;
    if (build_comm(level, nLayers, &cp)) return 1;
    unsigned mask; int nvar;
    if (halo_mask(varStart, varEnd, commPressure, commVisc, &mask, &nvar)) return 1;
    launch_halo_copy(g_tab[level], cp->local.blkA, cp->local.offA, cp->local.blkB, cp->local.offB, cp->local.n, mask, g_stream);
    for_level(level, [&](Block* b) { b->ss_valid = false; return 0; });
    return sync_and_check();
}

int adflow_gpu_halo_slot_info(int level, int nLayers, int isSend, int islot, int* peer, int* count)
{
    CommPattern* cp;
    if (build_comm(level, nLayers, &cp)) return 1;
    std::vector<CommList>& v = isSend ? cp->sends : cp->recvs;
    if (islot < 0 || islot >= (int)v.size()) {
        if (peer) *peer = -1;
        if (count) *count = 0;
        return 0;   // past the last slot: count 0
    }
    if (peer) *peer = v[islot].peer;
    if (count) *count = v[islot].n;
    return 0;
}

int adflow_gpu_halo_pack(int level, int nLayers, int islot, int varStart, int varEnd, int commPressure, int commVisc, double* buf)
{
    if (need_ready()) return 1;
    CommPattern* cp;
    if (build_comm(level, nLayers, &cp)) return 1;
    if (islot < 0 || islot >= (int)cp->sends.size()) return fail("send slot %d out of range", islot);
    unsigned mask; int nvar;
    if (halo_mask(varStart, varEnd, commPressure, commVisc, &mask, &nvar)) return 1;
    CommList& l = cp->sends[islot];
    launch_halo_pack(g_tab[level], l.blkA, l.offA, l.n, mask, l.buf, g_stream);
    HIPCHK(hipMemcpyAsync(buf, l.buf, sizeof(double) * (size_t)nvar * l.n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

int adflow_gpu_halo_unpack(int level, int nLayers, int islot, int varStart, int varEnd, int commPressure, int commVisc,
                           const double* buf)
{
    if (need_ready()) return 1;
    CommPattern* cp;
    if (build_comm(level, nLayers, &cp)) return 1;
    if (islot < 0 || islot >= (int)cp->recvs.size()) return fail("recv slot %d out of range", islot);
    unsigned mask; int nvar;
    if (halo_mask(varStart, varEnd, commPressure, commVisc, &mask, &nvar)) return 1;
    CommList& l = cp->recvs[islot];
    HIPCHK(hipMemcpyAsync(l.buf, buf, sizeof(double) * (size_t)nvar * l.n, hipMemcpyHostToDevice, g_stream));
    launch_halo_unpack(g_tab[level], l.blkA, l.offA, l.n, mask, l.buf, g_stream);
    HIPCHK(hipStreamSynchronize(g_stream));
    for_level(level, [&](Block* b) { b->ss_valid = false; return 0; });
    return 0;
}

static int comm_exchange_enqueue(CommPattern* cp, BlkView* tab, unsigned mask, int nvar);

// exchangePressureEarly (smoothers.F90:363-365, 674-676, multiGrid.F90:602-604): with the normal-momentum treatment of inviscid
// walls bcEulerWall reads the pressure of the first halo layer of the neighbouring blocks, so the reference exchanges the pressure
// alone -- whalo1(currentLevel, 1, 0, .true., .false., .false.) -- BEFORE applyAllBC, on the fine grid only
static int early_pressure_exchange_enqueue(int level)
{
    if (!g_opts.exchangePressureEarly || level > g_opts.groundLevel) return 0;
    if (!g_comm.count(std::make_pair(level, 1)))
        return fail("exchangePressureEarly: the 1-layer cell pattern of level %d (commPatternCell_1st / internalCell_1st) is not registered",
                    level);
    return halo_exchange_enqueue(level, 1, 0, 1, 0, 1);
}

static int halo_exchange_enqueue(int level, int varStart, int varEnd, int commPressure, int commVisc, int nLayers)
{
    CommPattern* cp;
    if (build_comm(level, nLayers, &cp)) return 1;
    unsigned mask; int nvar;
    if (halo_mask(varStart, varEnd, commPressure, commVisc, &mask, &nvar)) return 1;
    if (nvar == 0) return 0;
    if (comm_exchange_enqueue(cp, g_tab[level], mask, nvar)) return 1;
    return halo_exchange_close(level, varStart, varEnd, commPressure, nLayers);
}

// whalo2 closes by recomputing the total energy of the owned cells from p when both travelled (haloExchange.F90:178-196)
static int halo_exchange_close(int level, int varStart, int varEnd, int commPressure, int nLayers)
{
    const bool bothPAndE = commPressure && varStart <= 5 && varEnd >= 5;
    int nTodo = 0, nBlk = 0;
    for_level(level, [&](Block* b) {
        ++nBlk;
        if (nLayers == 2 && bothPAndE && !b->etot_consistent) ++nTodo;
        return 0;
    });
    if (nTodo > 0 && nTodo == nBlk) {
        LevelTab t;
        if (level_tab(level, &t)) return 1;
        launch_etot_owned_level(t.tab, t.n, t.nx, t.ny, t.nz, g_opts.gammaConstant, g_stream,
                                (g_etot_flag_level == level) ? g_floor_flag_dev : nullptr);
    }
    for_level(level, [&](Block* b) {
        // the exchange never touches owned cells: when their rhoE was produced by
        // computeEtotBlock already (stage update, or a previous whalo2) the pass is an identity
        if (nLayers == 2 && bothPAndE && !b->etot_consistent) {
            if (nTodo != nBlk) launch_etot_owned(b->v, g_opts.gammaConstant, g_stream);
            b->etot_consistent = true;
        }
        b->ss_valid = false;
        return 0;
    });
    return 0;
}

// pack -> grouped RCCL send/recv (own queue) || same-GPU copies -> unpack of the variables in `mask` over one pattern, in two halves:
// begin = everything up to the messages in flight and the same-GPU copies, end = the wait for the group, the unpacks and the periodic
// transformations.  The evaluation split around the exchange (block_res_split_enqueue) puts the halo-free tiles between the two.
static int comm_exchange_begin(CommPattern* cp, BlkView* tab, unsigned mask, int nvar, bool* remoteOut)
{
    // pack every outgoing message on the compute queue, then ONE grouped RCCL send/recv over xGMI on the communication queue;
    // the same-GPU copies (they read owned cells and write halos no message touches) run on the compute queue WHILE the
    // messages are in flight, the unpacks wait for the group (haloExchange.F90:553-719 does the same with isend / irecv /
    // local copy / waitany)
    for (auto& l : cp->sends) launch_halo_pack(tab, l.blkA, l.offA, l.n, mask, l.buf, g_stream);
    const bool remote = !cp->sends.empty() || !cp->recvs.empty();
    *remoteOut = remote;
    if (remote) {
#ifndef ADFLOW_NO_RCCL
        if (!g_nccl) return fail("halo exchange needs other ranks but adflow_gpu_comm_init was not called");
        hipStream_t sx = g_overlap ? g_streamX : g_stream;
        if (g_overlap) {
            HIPCHK(hipEventRecord(g_evPack, g_stream));
            HIPCHK(hipStreamWaitEvent(g_streamX, g_evPack, 0));
        }
        NCCLCHK(ncclGroupStart());
        for (auto& l : cp->sends)
            if (l.n > 0) NCCLCHK(ncclSend(l.buf, (size_t)nvar * l.n, ncclDouble, l.peer, g_nccl, sx));
        for (auto& l : cp->recvs)
            if (l.n > 0) NCCLCHK(ncclRecv(l.buf, (size_t)nvar * l.n, ncclDouble, l.peer, g_nccl, sx));
        NCCLCHK(ncclGroupEnd());
        if (g_overlap) HIPCHK(hipEventRecord(g_evComm, g_streamX));
#else
        return fail("built without RCCL: use adflow_gpu_halo_pack/unpack with an external transport");
#endif
    }
    launch_halo_copy(tab, cp->local.blkA, cp->local.offA, cp->local.blkB, cp->local.offB, cp->local.n, mask, g_stream);
    return 0;
}

static int comm_exchange_end(CommPattern* cp, BlkView* tab, unsigned mask, bool remote)
{
#ifndef ADFLOW_NO_RCCL
    if (remote && g_overlap) HIPCHK(hipStreamWaitEvent(g_stream, g_evComm, 0));
#endif
    (void)remote;
    for (auto& l : cp->recvs) launch_halo_unpack(tab, l.blkA, l.offA, l.n, mask, l.buf, g_stream);
    // periodic transformations of the halos that crossed a periodic interface: coordinates for the node pattern,
    // velocities when all three travelled (haloExchange.F90:456-457)
    const bool coor = (mask & (7u << 11)) != 0;
    const bool vel = (mask & 0xEu) == 0xEu;
    if (coor || vel)
        for (auto& pd : cp->periodic)
            launch_periodic(tab, pd.list.blkA, pd.list.offA, pd.list.n, pd.rotMatrix, pd.rotCenter, pd.translation, coor ? 1 : 0, g_stream);
    return 0;
}

static int comm_exchange_enqueue(CommPattern* cp, BlkView* tab, unsigned mask, int nvar)
{
    bool remote = false;
    if (comm_exchange_begin(cp, tab, mask, nvar, &remote)) return 1;
    return comm_exchange_end(cp, tab, mask, remote);
}

// exchangeCoor (haloExchange.F90:2456-2640): the three coordinates over the node pattern (nLayers key 0)
int adflow_gpu_exchange_coor(int level)
{
    if (need_ready()) return 1;
    CommPattern* cp;
    if (build_comm(level, 0, &cp)) return 1;
    if (comm_exchange_enqueue(cp, g_tab[level], 7u << 11, 3)) return 1;
    for_level(level, [&](Block* b) { b->face_vectors_valid = false; return 0; });
    return sync_and_check();
}

// xhalo_block (adjointExtra.F90:365-599) of every block of the level
int adflow_gpu_xhalo(int level)
{
    if (need_ready()) return 1;
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_xhalo_level(t.tab, t.n, t.nx, t.ny, t.nz, g_stream);
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    for (const BcPhase& ph : pl->ordinal) launch_xhalo_symm(t.tab, pl->d_ent, pl->d_order, ph, g_stream);
    for_level(level, [&](Block* b) { b->face_vectors_valid = false; return 0; });
    return sync_and_check();
}

int adflow_gpu_halo_exchange(int level, int varStart, int varEnd, int commPressure, int commVisc, int nLayers)
{
    if (need_ready()) return 1;
    if (halo_exchange_enqueue(level, varStart, varEnd, commPressure, commVisc, nLayers)) return 1;
    return sync_and_check();
}

// ----------------------------------------------------------------- smoothers
// one stage of either smoother after dw holds the scaled update: state update,
// boundary-condition hook, halo exchange (smoothers.F90:292-380, 600-691)
// updated: the state update ran inside the kernel that completed the increment (D-ADI k sweep)
static int finish_stage(int level, const KParams& kp, double scale, int fromWn, bool updated = false)
{
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    if (!updated) launch_stage_update_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, scale, fromWn, g_stream);
    int rc = for_level(level, [&](Block* b) {
        b->ss_valid = false;
        b->etot_consistent = true;
        return 0;
    });
    if (rc) return rc;
    const int secondHalo = (level <= g_opts.groundLevel);
    if (early_pressure_exchange_enqueue(level)) return 1;
    if (apply_bc_enqueue(level, secondHalo)) return 1;
    if (g_bc_callback) {
        HIPCHK(hipStreamSynchronize(g_stream));
        g_bc_callback(level, secondHalo);
    }
    const int nLayers = secondHalo ? 2 : 1;
    if (g_comm.count(std::make_pair(level, nLayers)))
        if (halo_exchange_enqueue(level, 1, 5, 1, 1, nLayers)) return 1;
    return 0;
}

static bool smooth_residual(int rkStage)
{
    if (g_opts.resAveraging == ADFLOW_RESAVG_NEVER) return false;
    if (g_opts.resAveraging == ADFLOW_RESAVG_ALWAYS) return true;
    return (rkStage % 2) == 1;
}

int adflow_gpu_rk_smooth(int level)
{
    if (need_ready()) return 1;
    if (g_opts.smoother != ADFLOW_RUNGE_KUTTA) return fail("adflow_gpu_rk_smooth called with smoother=%d", g_opts.smoother);
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    launch_rk_save_level(t.tab, t.n, t.nx, t.ny, t.nz, g_stream);
    const int nst = g_opts.nRKStages;
    for (int stage = 1; stage <= nst; ++stage) {
        KParams kp = make_kparams(level, 1.0, 1);
        const double scale = (g_opts.lowSpeedPreconditioner ? 0.8 : 1.0) * kp.cfl * g_opts.etaRK[stage - 1];   // smoothers.F90:202
        if (level_tab(level, &t)) return 1;      // a BC callback of the previous stage may have rebuilt the device table
        if (smooth_residual(stage)) {
            if (res_averaging_level(level, kp, scale)) return 1;
            if (finish_stage(level, kp, 0.0, 1)) return 1;
        } else {
            if (finish_stage(level, kp, scale, 1)) return 1;
        }
        if (stage < nst) {
            // residual of the next stage: rkStage = stage -> rFil = cdisRK(stage+1)
            KParams kr = make_kparams(level, g_opts.cdisRK[stage], 1);
            if (enqueue_flow_residual(level, kr, false, true, false)) return 1;
        }
    }
    return sync_and_check();
}

int adflow_gpu_dadi_smooth(int level)
{
    if (need_ready()) return 1;
    if (g_opts.smoother != ADFLOW_DADI) return fail("adflow_gpu_dadi_smooth called with smoother=%d", g_opts.smoother);
    const int nsub = (g_opts.groundLevel == 1) ? std::max(1, (int)g_opts.nSubiterations) : 1;
    for (int it = 1; it <= nsub; ++it) {
        KParams kp = make_kparams(level, 1.0, 0);
        LevelTab t;
        if (level_tab(level, &t)) return 1;
        const bool fuseUpd = !smooth_residual(0) && g_dadi_upd;               // (tuning "dadi_upd")
        launch_dadi_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, g_stream, fuseUpd);
        if (smooth_residual(0) && res_averaging_level(level, kp)) return 1;   // rkStage stays 0 under DADI
        if (finish_stage(level, kp, 0.0, 0, fuseUpd)) return 1;
        if (it < nsub) {
            if (enqueue_flow_residual(level, kp)) return 1;
        }
    }
    return sync_and_check();
}

// ---------------------------------------------------------------- multigrid
static int for_level_pairs(int fineLevel, const std::function<int(Block*, Block*)>& fn)
{
    bool any = false;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != fineLevel) continue;
        Block* c = find_block(std::get<2>(kv.first), fineLevel + 1, std::get<1>(kv.first));
        if (!c) return fail("block %d has no level-%d counterpart", std::get<2>(kv.first), fineLevel + 1);
        any = true;
        int rc = fn(kv.second, c);
        if (rc) return rc;
    }
    if (!any) return fail("no block registered on level %d", fineLevel);
    return 0;
}

static int exchange_if_registered(int level, int nLayers)
{
    if (g_comm.count(std::make_pair(level, nLayers))) return halo_exchange_enqueue(level, 1, 5, 1, 1, nLayers);
    return 0;
}

static double rfil_stage0(int* fwMode)
{
    *fwMode = (g_opts.smoother == ADFLOW_RUNGE_KUTTA) ? 1 : 0;
    return (g_opts.smoother == ADFLOW_RUNGE_KUTTA) ? g_opts.cdisRK[0] : 1.0;
}

static int transfer_to_coarse_enqueue(int level)
{
    const int cl = level + 1;
    int fwMode;
    const double rFil = rfil_stage0(&fwMode);
    // residual of the fine level with rkStage = 0 (multiGrid.F90:62-70)
    KParams kf = make_kparams(level, rFil, fwMode);
    kf.onlyRadii = 1;
    int rc = time_step_level(level, kf);
    if (rc) return rc;
    if (enqueue_flow_residual(level, kf)) return 1;
    // restriction + closures on the coarse level
    KParams kc = make_kparams(cl, rFil, fwMode);
    rc = for_level_pairs(level, [&](Block* f, Block* c) {
        if (!c->v.mgIFine || !c->v.mgIWeight) return fail("coarse block has no mgIFine/mgIWeight maps");
        if (!c->geom_uploaded) return fail("geometry of a level-%d block has not been uploaded", cl);
        c->ss_valid = false;
        c->etot_consistent = true;
        return 0;
    });
    if (rc) return rc;
    LevelTab tf, tc;
    if (level_tab(level, &tf) || level_tab(cl, &tc)) return 1;
    launch_restrict_level(tc.tab, tf.tab, tc.n, tc.nx, tc.ny, tc.nz, kc, g_stream);
    launch_corner_row_halos_level(tc.tab, tc.n, kc, g_stream);      // setCornerRowHalos(nwf) (multiGrid.F90:229)
    // applyAllBC(.false.) ; whalo1 (multiGrid.F90:236-241)
    if (apply_bc_enqueue(cl, 0)) return 1;
    if (g_bc_callback) {
        HIPCHK(hipStreamSynchronize(g_stream));
        g_bc_callback(cl, 0);
    }
    if (exchange_if_registered(cl, 1)) return 1;
    // time step, entry state, coarse residual from zero, forcing term (multiGrid.F90:246-320)
    kc.onlyRadii = 0;
    rc = time_step_level(cl, kc);
    if (rc) return rc;
    if (level_tab(cl, &tc)) return 1;       // BC registration may have rebuilt the table
    launch_store_entry_state_level(tc.tab, tc.n, tc.nx, tc.ny, tc.nz, g_stream);
    KParams kz = kc;
    kz.coarseInit = 0;
    if (enqueue_flow_residual(cl, kz)) return 1;
    launch_forcing_level(tc.tab, tc.n, tc.nx, tc.ny, tc.nz, g_opts.fcoll, g_stream);
    return 0;
}

static int transfer_to_fine_enqueue(int level)
{
    KParams kf = make_kparams(level, 1.0, 0);
    LevelTab tf, tc;
    if (level_tab(level, &tf) || level_tab(level + 1, &tc)) return 1;
    launch_corrections_level(tc.tab, tc.n, tc.nx, tc.ny, tc.nz, g_stream);
    int rc = for_level_pairs(level, [&](Block* f, Block* c) {
        if (!f->v.mgICoarse) return fail("fine block has no mgICoarse map");
        f->ss_valid = false;
        f->etot_consistent = true;
        return 0;
    });
    if (rc) return rc;
    // setCorrectionsCoarseHalos (multiGrid.F90:472): fact = 0, mgBoundCorr = bcDirichlet0 (inputParamRoutines.F90:3923)
    if (bc_coarse_corrections_enqueue(level + 1, 0.0)) return 1;
    launch_prolong_update_level(tf.tab, tc.tab, tc.n, tf.nx, tf.ny, tf.nz, kf, g_stream);
    const int secondHalo = (level <= g_opts.groundLevel);
    if (early_pressure_exchange_enqueue(level)) return 1;          // multiGrid.F90:602-604
    if (apply_bc_enqueue(level, secondHalo)) return 1;
    if (g_bc_callback) {
        HIPCHK(hipStreamSynchronize(g_stream));
        g_bc_callback(level, secondHalo);
    }
    return exchange_if_registered(level, secondHalo ? 2 : 1);
}

int adflow_gpu_transfer_to_coarse(int level)
{
    if (need_ready()) return 1;
    if (transfer_to_coarse_enqueue(level)) return 1;
    return sync_and_check();
}

int adflow_gpu_transfer_to_fine(int level)
{
    if (need_ready()) return 1;
    if (transfer_to_fine_enqueue(level)) return 1;
    return sync_and_check();
}

// coarseOwnedCoordinates(coarseLevel) (coarseUtils.F90:780-858) for every block pair (coarseLevel-1, coarseLevel)
int adflow_gpu_coarse_coordinates(int coarseLevel)
{
    if (need_ready()) return 1;
    if (coarseLevel < 2) return fail("coarse_coordinates: level %d has no finer level", coarseLevel);
    int rc = for_level_pairs(coarseLevel - 1, [&](Block* f, Block* c) {
        (void)f;
        if (!c->v.mgIFine) return fail("coarse block has no mgIFine maps");
        c->face_vectors_valid = false;
        return 0;
    });
    if (rc) return rc;
    LevelTab tf, tc;
    if (level_tab(coarseLevel - 1, &tf) || level_tab(coarseLevel, &tc)) return 1;
    launch_coarse_coordinates_level(tc.tab, tf.tab, tc.n, tc.nx, tc.ny, tc.nz, g_stream);
    return sync_and_check();
}

// executeMGCycle as ONE hipGraph.  A cycle enqueues ~10^3 kernels and most of them (the coarse levels) run 10 - 40 us: the launch
// gaps, not the kernels, bound them (profiles/r02_br_mg_trace.md).  Everything a cycle enqueues is fixed by the options, the tuning,
// the registered blocks / patterns / subfaces and the cycling strategy, so the third identical call in a row (the first warms the
// caches, no allocation may happen under capture; the second is captured) replays the graph.  Not captured: host callbacks
// (boundary-condition hooks), phase events, actuator regions (their relaxation factor changes from cycle to cycle), RCCL messages.
namespace {
struct MgGraph {
    std::vector<int32_t> cyc;
    long gen = -1;
    int seen = 0;                   // identical calls in a row that ran directly
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph = nullptr;
    bool failed = false;            // capture or instantiation failed once: direct enqueue from then on
    // what is enqueued also depends on the blocks' host-side flags (a stale sensor adds a k_entropy pass, ...): the graph is valid
    // for the flags it was captured from (pre) and leaves the flags of the end of the captured cycle (post)
    std::vector<unsigned char> pre, post;
};
MgGraph g_mgg;

void mg_graph_drop()
{
    if (g_mgg.exec) (void)hipGraphExecDestroy(g_mgg.exec);
    if (g_mgg.graph) (void)hipGraphDestroy(g_mgg.graph);
    g_mgg.exec = nullptr; g_mgg.graph = nullptr; g_mgg.seen = 0; g_mgg.gen = -1; g_mgg.cyc.clear();
}

static std::vector<unsigned char> block_flags()
{
    std::vector<unsigned char> f;
    for (auto& kv : g_blocks) {
        const Block* b = kv.second;
        f.push_back((unsigned char)(b->geom_uploaded | (b->normals_from_x_ok << 1) | (b->face_vectors_valid << 2) | (b->ss_valid << 3) |
                                    (b->etot_consistent << 4)));
    }
    return f;
}

void set_block_flags(const std::vector<unsigned char>& f)
{
    size_t q = 0;
    for (auto& kv : g_blocks) {
        if (q >= f.size()) break;
        Block* b = kv.second;
        const unsigned char v = f[q++];
        b->geom_uploaded = v & 1; b->normals_from_x_ok = (v >> 1) & 1; b->face_vectors_valid = (v >> 2) & 1; b->ss_valid = (v >> 3) & 1;
        b->etot_consistent = (v >> 4) & 1;
    }
}

bool mg_graph_eligible()
{
#ifdef HOSTSIM
    return false;
#else
    if (!g_mg_graph || g_mgg.failed || g_bc_callback || g_turb_bc_callback || g_phase_base > 0 || !g_act.empty()) return false;
    for (auto& kv : g_comm)
        if (!kv.second.h_sendProc.empty() || !kv.second.h_recvProc.empty() || g_comm_self) return false;
    return true;
#endif
}
}  // namespace

static int mg_cycle_enqueue(const int32_t* cycling, int nSteps);

int adflow_gpu_mg_cycle(const int32_t* cycling, int nSteps)
{
    if (need_ready()) return 1;
    if (!cycling || nSteps < 1) return fail("mg_cycle: empty cycling strategy");
#ifndef HOSTSIM
    if (mg_graph_eligible()) {
        const bool same = (g_mgg.gen == g_state_gen && (int)g_mgg.cyc.size() == nSteps && !memcmp(g_mgg.cyc.data(), cycling, sizeof(int32_t) * nSteps));
        if (!same) {
            mg_graph_drop();
            g_mgg.cyc.assign(cycling, cycling + nSteps);
            g_mgg.gen = g_state_gen;
        }
        if (g_mgg.exec && block_flags() == g_mgg.pre) {
            HIPCHK(hipGraphLaunch(g_mgg.exec, g_stream));
            set_block_flags(g_mgg.post);
            return sync_and_check();
        }
        if (g_mgg.exec) {           // other flags than the captured cycle started from: this call runs directly
            g_mgg.seen = 0;
        } else if (g_mgg.seen >= 1) {
            // the previous identical call ran directly (every cache is warm): capture this one
            HIPCHK(hipStreamSynchronize(g_stream));
            g_mgg.pre = block_flags();
            if (hipStreamBeginCapture(g_stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const bool was = g_async;
                g_async = true;
                const int rc = mg_cycle_enqueue(cycling, nSteps);
                g_async = was;
                hipGraph_t gr = nullptr;
                const hipError_t e1 = hipStreamEndCapture(g_stream, &gr);
                if (rc == 0 && e1 == hipSuccess && gr && !(g_test_fault & 1) && hipGraphInstantiate(&g_mgg.exec, gr, nullptr, nullptr, 0) == hipSuccess) {
                    g_mgg.graph = gr;
                    g_mgg.post = block_flags();
                    HIPCHK(hipGraphLaunch(g_mgg.exec, g_stream));
                    return sync_and_check();
                }
                // capture failed: nothing was executed, but the enqueue walked the host-side block flags (ss_valid, etot_consistent,
                // face_vectors_valid) to their post-cycle values: put them back, then run the cycle directly -- for good, and also
                // when the enqueue itself reported an error under capture (the direct path reports it again if it is a real one)
                if (gr) (void)hipGraphDestroy(gr);
                (void)hipGetLastError();
                g_mgg.exec = nullptr;
                g_mgg.failed = true;
                set_block_flags(g_mgg.pre);
            } else {
                (void)hipGetLastError();
                g_mgg.failed = true;
            }
        }
        ++g_mgg.seen;
    }
#endif
    const bool was_async = g_async;
    g_async = true;                 // the whole cycle is enqueued, one sync at the end
    const int rc = mg_cycle_enqueue(cycling, nSteps);
    g_async = was_async;
    if (rc) return rc;
    return sync_and_check();
}

static int mg_cycle_enqueue(const int32_t* cycling, int nSteps)
{
    int level = g_opts.groundLevel;
    int rc = 0;
    for (int n = 0; n < nSteps && !rc; ++n) {
        switch (cycling[n]) {
        case -1:
            level -= 1;
            rc = transfer_to_fine_enqueue(level);
            break;
        case 0: {
            if (n > 0 && cycling[n - 1] != 1) {
                // time step + residual with rkStage = 0 (multiGrid.F90:880-888)
                int fwMode;
                const double rFil = rfil_stage0(&fwMode);
                KParams kp = make_kparams(level, rFil, fwMode);
                rc = time_step_level(level, kp);
                if (!rc) rc = enqueue_flow_residual(level, kp);
            }
            if (!rc) rc = (g_opts.smoother == ADFLOW_RUNGE_KUTTA) ? adflow_gpu_rk_smooth(level) : adflow_gpu_dadi_smooth(level);
            break;
        }
        case 1:
            rc = transfer_to_coarse_enqueue(level);
            level += 1;
            break;
        default:
            rc = fail("mg_cycle: cycling(%d) = %d is not -1, 0 or 1", n + 1, cycling[n]);
        }
    }
    if (!rc && g_opts.equations == ADFLOW_RANS) {
        // turbSolveDDADI on the ground level (multiGrid.F90:938)
        rc = adflow_gpu_sa_solve(g_opts.groundLevel);
    }
    if (!rc) {
        // closing time step + residual on the ground level (multiGrid.F90:944-950)
        level = g_opts.groundLevel;
        int fwMode;
        const double rFil = rfil_stage0(&fwMode);
        KParams kp = make_kparams(level, rFil, fwMode);
        rc = time_step_level(level, kp);
        if (!rc) rc = enqueue_flow_residual(level, kp);
    }
    return rc;
}

// --------------------------------------------------------- Newton-Krylov glue
namespace {
double* g_vec_dev = nullptr;     // device staging of the PETSc-layout vectors
size_t g_vec_elems = 0;

int vec_reserve(size_t n)
{
    if (n <= g_vec_elems) return 0;
    if (g_vec_dev) (void)hipFree(g_vec_dev);
    g_vec_dev = nullptr;
    g_vec_elems = 0;
    HIPCHK(hipMalloc((void**)&g_vec_dev, n * sizeof(double)));
    g_vec_elems = n;
    return 0;
}

long level1_dof(void)
{
    long n = 0;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == 1) n += (long)kv.second->v.nx * kv.second->v.ny * kv.second->v.nz * kv.second->v.nw;
    return n;
}

// blocks in the reference's vector order: nn ascending (sps = 1)
int for_level1_in_order(const std::function<int(Block*, long)>& fn)
{
    std::map<int, Block*> byNN;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == 1 && std::get<1>(kv.first) == 1) byNN[std::get<2>(kv.first)] = kv.second;
    if (byNN.empty()) return fail("no block registered on level 1");
    long off = 0;
    for (auto& kv : byNN) {
        int rc = fn(kv.second, off);
        if (rc) return rc;
        off += (long)kv.second->v.nx * kv.second->v.ny * kv.second->v.nz * kv.second->v.nw;
    }
    return 0;
}

// The staging of a host form: its vectors of n doubles side by side in `base` (g_vec_dev, or an allocation of the call), vector q at
// s[q].  A host form is: its argument check, stage_open, in(), the enqueue function its _dev twin calls, out(), done() -- the one
// synchronise, whatever adflow_gpu_set_async says.
struct Stage {
    long n = 0;
    double* base = nullptr;
    mutable bool pending = false;      // a copy from or into one of the caller's host arrays is in the queue
    // an exit in front of done() (a refusal after in()): the caller's arrays are not read or written once the entry has returned
    ~Stage() { if (pending) (void)hipStreamSynchronize(g_stream); }
    double* operator[](int q) const { return base + (size_t)q * n; }
    int in(int q, const double* h) const
    {
        HIPCHK(hipMemcpyAsync((*this)[q], h, sizeof(double) * n, hipMemcpyHostToDevice, g_stream));
        pending = true;
        return 0;
    }
    int out(double* h, int q) const { return scalars(h, (*this)[q], n); }
    int scalars(double* h, const double* d, long count) const
    {
        HIPCHK(hipMemcpyAsync(h, d, sizeof(double) * count, hipMemcpyDeviceToHost, g_stream));
        pending = true;
        return 0;
    }
    int done() const
    {
        HIPCHK(hipStreamSynchronize(g_stream));
        pending = false;
        return 0;
    }
};

int stage_open(Stage* s, long n, int nvec)
{
    if (vec_reserve((size_t)nvec * n)) return 1;
    s->n = n;
    s->base = g_vec_dev;
    return 0;
}

// the flag the closures of a state write raise where they floored a pressure: there, and cleared on the stream
int floor_flag_clear()
{
    if (!g_floor_flag_dev) HIPCHK(hipMalloc((void**)&g_floor_flag_dev, sizeof(int)));
    HIPCHK(hipMemsetAsync(g_floor_flag_dev, 0, sizeof(int), g_stream));
    return 0;
}

// a state write moved the flow variables of level 1: the sensor and the energy / pressure consistency of its blocks no longer hold
int flow_state_written()
{
    return for_level1_in_order([&](Block* b, long) {
        b->ss_valid = false;
        b->etot_consistent = false;
        return 0;
    });
}

int set_w_dev(const double* d_vec, bool withClosures = false)
{
    const double turbFloor = 1e-6 * g_opts.wInf[5];
    LevelTab t;
    if (level_tab(1, &t)) return 1;
    // block offsets: BlkView::vecOff; withClosures: the closures blocketteRes would start with, in the same pass
    if (withClosures) {
        KParams kp = make_kparams(1, 1.0, 0);
        if (floor_flag_clear()) return 1;
        launch_set_w_closures_level(t.tab, t.n, t.nx, t.ny, t.nz, d_vec, turbFloor, kp, g_floor_flag_dev, g_stream);
    } else
        launch_set_w_level(t.tab, t.n, t.nx, t.ny, t.nz, d_vec, turbFloor, g_stream);
    return flow_state_written();
}

int get_r_dev(double* d_vec, double turbScale, double* d_sums)
{
    LevelTab t;
    if (level_tab(1, &t)) return 1;
    launch_get_r_level(t.tab, t.n, t.nx, t.ny, t.nz, d_vec, turbScale, d_sums, g_stream);
    return 0;
}
}  // namespace

int adflow_gpu_set_w_vec(const double* wVec, long n)
{
    if (need_ready()) return 1;
    if (!wVec || n != level1_dof()) return fail("set_w_vec: n=%ld but the level-1 blocks hold %ld DOF", n, level1_dof());
    Stage s;
    return stage_open(&s, n, 1) || s.in(0, wVec) || set_w_dev(s[0]) || s.done();
}

static int get_vec_common(double* out, long n, double turbScale, double* sumsq2)
{
    if (need_ready()) return 1;
    if (!out || n != level1_dof()) return fail("get_r_vec: n=%ld but the level-1 blocks hold %ld DOF", n, level1_dof());
    Stage s;
    if (stage_open(&s, n, 1)) return 1;
    if (!g_norm_dev) HIPCHK(hipMalloc((void**)&g_norm_dev, sizeof(double) * 8));
    HIPCHK(hipMemsetAsync(g_norm_dev, 0, sizeof(double) * 8, g_stream));
    if (get_r_dev(s[0], turbScale, sumsq2 ? g_norm_dev : nullptr) || s.out(out, 0)) return 1;
    return (sumsq2 && s.scalars(sumsq2, g_norm_dev, 2)) || s.done();
}

int adflow_gpu_get_r_vec(double* rVec, long n, double* sumsq2) { return get_vec_common(rVec, n, g_opts.turbResScale, sumsq2); }
int adflow_gpu_get_res(double* res, long n) { return get_vec_common(res, n, 1.0, nullptr); }

static int nk_core_enqueue(bool closuresDone = false)
{
    // blocketteRes with its default arguments (blockette.F90:130-160): exact residual,
    // flow + turbulence, no intermediate update
    unsigned flags = (closuresDone ? 0u : ADFLOW_RES_CLOSURES) | ADFLOW_RES_HALO | ADFLOW_RES_FLOW;
    if (g_opts.equations == ADFLOW_RANS) flags |= ADFLOW_RES_TURB;
    return block_res_enqueue(1, flags);
}

// FormFunction_mf on device vectors (d_rVec may be d_wVec: every entry of w is consumed by setW before the first residual kernel starts)
static int nk_residual_enqueue(const double* d_wVec, double* d_rVec)
{
    if (set_w_dev(d_wVec, true)) return 1;
    g_etot_flag_level = 1;      // the owned energy is computeEtot(p) already wherever p kept its value (k_set_w_closures_level)
    // setRVec rides on the kernels that complete dw (Roe march, SA march) where those run; otherwise its own pass.  Actuator
    // sources are added to dw behind the core: then the vector is taken from dw afterwards.
    g_rvec_done = 0;
    g_rvec_target = g_act.empty() ? d_rVec : nullptr;
    const int rc = nk_core_enqueue(true);
    g_rvec_target = nullptr;
    g_etot_flag_level = 0;
    if (rc) return rc;
    const int need = (g_opts.equations == ADFLOW_RANS) ? 3 : 1;
    if ((g_rvec_done & need) != need)
        if (get_r_dev(d_rVec, g_opts.turbResScale, nullptr)) return 1;
    return 0;
}

int adflow_gpu_nk_residual_dev(const double* d_wVec, double* d_rVec, long n)
{
    if (need_ready()) return 1;
    if (!d_wVec || !d_rVec || n != level1_dof()) return fail("nk_residual: n=%ld but the level-1 blocks hold %ld DOF", n, level1_dof());
    if (nk_residual_enqueue(d_wVec, d_rVec)) return 1;
    return sync_and_check();
}

int adflow_gpu_nk_residual(const double* wVec, double* rVec, long n)
{
    if (need_ready()) return 1;
    if (!wVec || !rVec || n != level1_dof()) return fail("nk_residual: n=%ld but the level-1 blocks hold %ld DOF", n, level1_dof());
    Stage s;                           // one buffer for w and r (see nk_residual_enqueue)
    return stage_open(&s, n, 1) || s.in(0, wVec) || nk_residual_enqueue(s[0], s[0]) || s.out(rVec, 0) || s.done();
}

// ---- products with the assembled matrix (kernels_jacmult.hip): y = J x, y = J^T x on PETSc-layout device vectors ----------------
// MatMult on the matrices of setupStateResidualMatrix: solveAdjoint's GMRES on dRdwT (adjointAPI.F90:661-863, :741, :806).
namespace {
struct JmWork {
    int level = 0, nState = 0, nslots = 0, nx = 0, ny = 0, nz = 0;
    int nv = 0;                        // vectors xs and ys hold side by side: 1 until a multi-vector product asked for more
    long ndof = 0;                     // nState x owned cells of the level
    long zeroGen = -1;                 // g_state_gen at which the halos of xs were last cleared
    size_t bytes = 0;
    std::vector<long> sig;             // what the work space was laid out for
    std::vector<void*> raw;            // one allocation per block: xs, ys (nv vectors of nState components each)
    std::vector<JmBlk> h;              // host copy of the table, indexed by nn
    // nv tables each, one behind the other, table v with xs / ys of vector v (the kernels that take one vector run on any of them)
    JmBlk* tab = nullptr;
    BlkView *tabX = nullptr, *tabY = nullptr;    // the level's block table with w -> xs / ys: the halo kernels on a foreign array
    size_t slots() const { return h.size(); }
};
JmWork g_jm;                           // the products with the assembled matrix
JmWork g_jf;                           // the matrix-free products (adflow_gpu_jacfree_mult): xs and its tables only, no matrix
}  // namespace

static int64_t jm_release_work(JmWork& W)
{
    const int64_t n = (int64_t)W.bytes;
    for (void* p : W.raw) (void)hipFree(p);
    if (W.tab) (void)hipFree(W.tab);
    if (W.tabX) (void)hipFree(W.tabX);
    if (W.tabY) (void)hipFree(W.tabY);
    W = JmWork();
    return n;
}
static int64_t jm_release() { return jm_release_work(g_jm) + jm_release_work(g_jf); }

// scratch arrays and tables of the product on `level` for nv vectors at once (kept between calls at the widest nv asked for; laid out
// again when blocks or matrix changed).  matrix: W serves the assembled matrix g_jac (its blocks in the table, xs and ys); otherwise
// the matrix-free product of nS variables per cell: the same halo'd xs and tables, no blocks and no ys
static int jm_layout(JmWork& W, int level, int nS, int nv, bool matrix, const char* who)
{
    std::vector<long> sig = {level, nS};
    int maxnn = 0;
    int rc = for_level(level, [&](Block* b) {
        if (matrix && (!b->jac || b->jac_ncomp != g_jac.nStencil * nS * nS))
            return fail("%s: a block of level %d has no assembled blocks (registered after the assembly?)", who, level);
        if (matrix && (double)b->v.nbox * nS * nS * 8.0 >= 4294967296.0)
            return fail("%s: block of %ld box cells: nState^2 planes exceed the 4 GiB the kernels address from one base", who, b->v.nbox);
        return 0;
    });
    if (rc) return rc;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level) {
            sig.push_back(std::get<2>(kv.first)); sig.push_back((long)(intptr_t)kv.second);
            sig.push_back(matrix ? (long)(intptr_t)kv.second->jac : 0);
            sig.push_back(kv.second->v.nbox);
            maxnn = std::max(maxnn, std::get<2>(kv.first));
        }
    if (W.tab && sig == W.sig && nv <= W.nv) return 0;
    if (W.tab && sig == W.sig) nv = std::max(nv, W.nv);
    HIPCHK(hipStreamSynchronize(g_stream));
    (void)jm_release_work(W);
    const int halves = matrix ? 2 : 1;                                    // xs and ys, or xs alone
    W.level = level; W.nState = nS; W.nslots = maxnn; W.nv = nv;
    W.h.assign(maxnn + 1, JmBlk());
    memset(W.h.data(), 0, sizeof(JmBlk) * W.h.size());
    const size_t nt = (size_t)maxnn + 1;
    std::vector<BlkView> hx(nt * nv), hy(nt * nv);
    memset(hx.data(), 0, sizeof(BlkView) * hx.size());
    memset(hy.data(), 0, sizeof(BlkView) * hy.size());
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level) continue;
        Block* b = kv.second;
        const BlkView& v = b->v;
        const size_t bytes = (size_t)v.nbox * halves * nS * nv * sizeof(double) + 256;
        void* raw = nullptr;
        if (hipMalloc(&raw, bytes) != hipSuccess) {
            (void)hipGetLastError();
            (void)jm_release_work(W);
            return fail("%s: cannot allocate %zu bytes of scratch for %d vectors on a block of %ld box cells", who, bytes, nv, v.nbox);
        }
        W.raw.push_back(raw);
        W.bytes += bytes;
        HIPCHK(hipMemsetAsync(raw, 0, bytes, g_stream));
        JmBlk& q = W.h[std::get<2>(kv.first)];
        q.nx = v.nx; q.ny = v.ny; q.nz = v.nz; q.il = v.il; q.jl = v.jl; q.kl = v.kl; q.ib = v.ib; q.jb = v.jb; q.kb = v.kb;
        q.ldi = v.ldi; q.ldk = v.ldk; q.nbox = v.nbox;
        q.jac = matrix ? b->jac : nullptr;
        q.xs = (double*)raw + ADF_PAD0;
        q.ys = matrix ? q.xs + (size_t)v.nbox * nS * nv : nullptr;
        for (int c = 0; c < nv; ++c) {
            BlkView &x = hx[c * nt + std::get<2>(kv.first)], &y = hy[c * nt + std::get<2>(kv.first)];
            x = v; x.w = q.xs + (size_t)v.nbox * nS * c;
            y = v; y.w = matrix ? q.ys + (size_t)v.nbox * nS * c : nullptr;
        }
        W.nx = std::max(W.nx, v.nx); W.ny = std::max(W.ny, v.ny); W.nz = std::max(W.nz, v.nz);
    }
    long off = 0;                     // PETSc vector order: block nn ascending (NKSolvers.F90:1240-1253), nState entries per cell
    for (auto& q : W.h) { q.vecOff = off; off += (long)q.nx * q.ny * q.nz * nS; }
    W.ndof = off;
    std::vector<JmBlk> ht(nt * nv);
    for (int c = 0; c < nv; ++c)
        for (size_t q = 0; q < nt; ++q) {
            JmBlk& t = ht[c * nt + q];
            t = W.h[q];
            if (t.xs) t.xs += (size_t)t.nbox * nS * c;
            if (t.ys) t.ys += (size_t)t.nbox * nS * c;
        }
    if (hipMalloc((void**)&W.tab, sizeof(JmBlk) * ht.size()) != hipSuccess ||
        hipMalloc((void**)&W.tabX, sizeof(BlkView) * hx.size()) != hipSuccess ||
        hipMalloc((void**)&W.tabY, sizeof(BlkView) * hy.size()) != hipSuccess) {
        (void)hipGetLastError();
        (void)jm_release_work(W);           // the scratch arrays as well: a later call lays everything out again
        return fail("%s: cannot allocate the block tables of %d vectors (%zu blocks); no scratch is held", who, nv, nt);
    }
    HIPCHK(hipMemcpy(W.tab, ht.data(), sizeof(JmBlk) * ht.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(W.tabX, hx.data(), sizeof(BlkView) * hx.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(W.tabY, hy.data(), sizeof(BlkView) * hy.size(), hipMemcpyHostToDevice));
    W.sig = sig;
    W.zeroGen = g_state_gen;
    return 0;
}
static int jm_prepare(int level, int nv = 1) { return jm_layout(g_jm, level, g_jac.nState, nv, true, "jacobian_mult"); }

// one reverse exchange as a donor-sorted list: targets (tb, to) with sources (sb, so), or with the position in the message
static int jm_acc_build(JmAccList& a, const int* d_tBlk, const long* d_tOff, const int* d_sBlk, const long* d_sOff, int n)
{
    a = JmAccList();
    if (n <= 0) return 0;
    std::vector<int> tb(n), sb(n);
    std::vector<long> to(n), so(n);
    HIPCHK(hipMemcpy(tb.data(), d_tBlk, sizeof(int) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(to.data(), d_tOff, sizeof(long) * n, hipMemcpyDeviceToHost));
    if (d_sBlk) {
        HIPCHK(hipMemcpy(sb.data(), d_sBlk, sizeof(int) * n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(so.data(), d_sOff, sizeof(long) * n, hipMemcpyDeviceToHost));
    } else
        for (int t = 0; t < n; ++t) { sb[t] = t; so[t] = 0; }
    std::vector<int> perm(n);
    for (int t = 0; t < n; ++t) perm[t] = t;
    std::sort(perm.begin(), perm.end(), [&](int p, int q) {
        if (tb[p] != tb[q]) return tb[p] < tb[q];
        if (to[p] != to[q]) return to[p] < to[q];
        if (sb[p] != sb[q]) return sb[p] < sb[q];
        return so[p] < so[q];
    });
    std::vector<int> utb, seg, ssb(n);
    std::vector<long> uto, sso(n);
    for (int e = 0; e < n; ++e) {
        const int t = perm[e];
        if (e == 0 || tb[t] != utb.back() || to[t] != uto.back()) { utb.push_back(tb[t]); uto.push_back(to[t]); seg.push_back(e); }
        ssb[e] = sb[t]; sso[e] = so[t];
    }
    seg.push_back(n);
    a.nu = (int)utb.size(); a.nsrc = n;
    HIPCHK(hipMalloc((void**)&a.tBlk, sizeof(int) * a.nu));
    HIPCHK(hipMalloc((void**)&a.tOff, sizeof(long) * a.nu));
    HIPCHK(hipMalloc((void**)&a.seg, sizeof(int) * (a.nu + 1)));
    HIPCHK(hipMalloc((void**)&a.sBlk, sizeof(int) * n));
    HIPCHK(hipMemcpy(a.tBlk, utb.data(), sizeof(int) * a.nu, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(a.tOff, uto.data(), sizeof(long) * a.nu, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(a.seg, seg.data(), sizeof(int) * (a.nu + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(a.sBlk, ssb.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    if (d_sBlk) {
        HIPCHK(hipMalloc((void**)&a.sOff, sizeof(long) * n));
        HIPCHK(hipMemcpy(a.sOff, sso.data(), sizeof(long) * n, hipMemcpyHostToDevice));
    }
    return 0;
}

static int jm_acc_lists(CommPattern* cp)
{
    if (cp->accBuilt) return 0;
    for (auto& a : cp->acc) free_acc_list(a);
    cp->acc.assign(1 + cp->sends.size(), JmAccList());
    if (jm_acc_build(cp->acc[0], cp->local.blkA, cp->local.offA, cp->local.blkB, cp->local.offB, cp->local.n)) return 1;
    for (size_t i = 0; i < cp->sends.size(); ++i)
        if (jm_acc_build(cp->acc[1 + i], cp->sends[i].blkA, cp->sends[i].offA, nullptr, nullptr, cp->sends[i].n)) return 1;
    cp->accBuilt = true;
    return 0;
}

// the registered 2-layer cell pattern of the level, or NULL when there is none (then no halo has a donor).  A rotational
// periodicity would have to turn the velocity entries of the halos (forward: rotMatrix, reverse: its transpose): refused
static int jm_pattern_of(int level, int lStart, int nState, const char* who, CommPattern** out)
{
    *out = nullptr;
    if (!g_comm.count(std::make_pair(level, 2))) return 0;
    if (build_comm(level, 2, out)) return 1;
    if (lStart == 0 && nState >= 5)
        for (auto& pd : (*out)->periodic) {
            bool identity = true;
            for (int q = 0; q < 9; ++q)
                if (pd.rotMatrix[q] != ((q % 4 == 0) ? 1.0 : 0.0)) identity = false;
            if (!identity && !pd.h_block.empty())
                return fail("%s: rotational periodicity is not supported by the product (a registered periodic transformation of "
                            "level %d rotates the velocities of its halos)", who, level);
        }
    return 0;
}
static int jm_pattern(int level, CommPattern** out) { return jm_pattern_of(level, g_jac.lStart, g_jac.nState, "jacobian_mult", out); }

// the owned entries of the nv vectors into the halo'd arrays xs of W (halos without a donor read as zero) ...
static int jm_scatter_x(JmWork& W, const double* d_x, int nv, long ldx)
{
    const int nS = W.nState;
    const size_t nt = W.slots();
    if (W.zeroGen != g_state_gen) {
        // patterns may have changed: a halo that lost its donor must read as zero again
        for (auto& q : W.h)
            if (q.xs) HIPCHK(hipMemsetAsync(q.xs - ADF_PAD0, 0, ((size_t)q.nbox * nS * W.nv + ADF_PAD0) * sizeof(double), g_stream));
        W.zeroGen = g_state_gen;
    }
    for (int v = 0; v < nv; ++v) launch_jm_scatter(W.tab + v * nt, W.nslots, W.nx, W.ny, W.nz, nS, d_x + v * ldx, g_stream);
    return 0;
}
// ... and the 2-layer exchange on them: every halo with a donor takes its donor's entries
static int jm_exchange_x(JmWork& W, CommPattern* cp, int nv)
{
    const int nS = W.nState;
    const unsigned mask = (1u << nS) - 1u;
    const size_t nt = W.slots();
    for (int v = 0; cp && v < nv; ++v) {
        bool remote = false;
        if (comm_exchange_begin(cp, W.tabX + v * nt, mask, nS, &remote)) return 1;
#ifndef ADFLOW_NO_RCCL
        if (remote && g_overlap) HIPCHK(hipStreamWaitEvent(g_stream, g_evComm, 0));
#endif
        for (auto& l : cp->recvs) launch_halo_unpack(W.tabX + v * nt, l.blkA, l.offA, l.n, mask, l.buf, g_stream);
    }
    return 0;
}

// y = J x (J^T x) for nv = 1 .. JM_MAXW vectors in one pass over the matrix: column v of x and y starts v ldx / v ldy doubles behind
// column 0.  The vectors travel through the scratch arrays, the exchange and the reverse accumulation one at a time with the kernels
// of one vector (the halo is small); the product kernels read every block once for all of them
static int jm_mult_enqueue(int level, int transpose, const double* d_x, double* d_y, int nv = 1, long ldx = 0, long ldy = 0)
{
    if (jm_prepare(level, nv)) return 1;
    CommPattern* cp;
    if (jm_pattern(level, &cp)) return 1;
    const int nS = g_jm.nState;
    const unsigned mask = (1u << nS) - 1u;
    const size_t nt = g_jm.slots();
    JmStencil S;
    S.n = g_jac.nStencil;
    for (int s = 0; s < S.n; ++s)
        for (int d = 0; d < 3; ++d) {
            S.d[s][d] = g_jac.st[s][d];
            if (S.d[s][d] < -2 || S.d[s][d] > 2) return fail("jacobian_mult: stencil offset beyond the two halo layers");
        }
    if (jm_scatter_x(g_jm, d_x, nv, ldx)) return 1;
    if (!transpose) {
        if (jm_exchange_x(g_jm, cp, nv)) return 1;
        launch_jac_mult(g_jm.tab, g_jm.nslots, g_jm.nx, g_jm.ny, g_jm.nz, nS, S, d_y, g_stream, nv, ldy);
        return 0;
    }
    launch_jac_mult_t(g_jm.tab, g_jm.nslots, g_jm.nx, g_jm.ny, g_jm.nz, nS, S, g_stream, nv);
    if (cp && jm_acc_lists(cp)) return 1;
    for (int v = 0; cp && v < nv; ++v) {
        const JmBlk* tab = g_jm.tab + v * nt;
        // the messages of the forward exchange the other way: the halos of the receive lists go back to the ranks they came from
        for (auto& l : cp->recvs) launch_halo_pack(g_jm.tabY + v * nt, l.blkA, l.offA, l.n, mask, l.buf, g_stream);
        const bool remote = !cp->sends.empty() || !cp->recvs.empty();
        if (remote) {
#ifndef ADFLOW_NO_RCCL
            if (!g_nccl) return fail("jacobian_mult needs other ranks but adflow_gpu_comm_init was not called");
            hipStream_t sx = g_overlap ? g_streamX : g_stream;
            if (g_overlap) {
                HIPCHK(hipEventRecord(g_evPack, g_stream));
                HIPCHK(hipStreamWaitEvent(g_streamX, g_evPack, 0));
            }
            NCCLCHK(ncclGroupStart());
            for (auto& l : cp->recvs)
                if (l.n > 0) NCCLCHK(ncclSend(l.buf, (size_t)nS * l.n, ncclDouble, l.peer, g_nccl, sx));
            for (auto& l : cp->sends)
                if (l.n > 0) NCCLCHK(ncclRecv(l.buf, (size_t)nS * l.n, ncclDouble, l.peer, g_nccl, sx));
            NCCLCHK(ncclGroupEnd());
            if (g_overlap) HIPCHK(hipEventRecord(g_evComm, g_streamX));
#else
            return fail("built without RCCL: the product across ranks needs it");
#endif
        }
        // same-process pairs while the messages are in flight, then the messages in the order of the send lists: every donor is
        // updated by one lane per list, the lists one after the other
        launch_jac_halo_accumulate(tab, cp->acc[0], nS, nullptr, 0, g_stream);
#ifndef ADFLOW_NO_RCCL
        if (remote && g_overlap) HIPCHK(hipStreamWaitEvent(g_stream, g_evComm, 0));
#endif
        for (size_t i = 0; i < cp->sends.size(); ++i)
            launch_jac_halo_accumulate(tab, cp->acc[1 + i], nS, cp->sends[i].buf, cp->sends[i].n, g_stream);
    }
    for (int v = 0; v < nv; ++v)
        launch_jm_gather(g_jm.tab + v * nt, g_jm.nslots, g_jm.nx, g_jm.ny, g_jm.nz, nS, d_y + v * ldy, g_stream);
    return 0;
}

static int jm_check(int level, const double* x, const double* y, long n, const char* who = "jacobian_mult")
{
    if (need_ready()) return 1;
    if (!g_jac_valid) return fail("%s: no assembled Jacobian (call adflow_gpu_fd_jacobian first)", who);
    if (level != g_jac_level) return fail("%s: level %d is not the level of the assembly (%d)", who, level, g_jac_level);
    if (!x || !y) return fail("%s: %s is NULL", who, !x ? "x" : "y");
    if (x == y) return fail("%s: x and y are the same vector (the product is not done in place)", who);
    long cells = 0;
    int rc = for_level(level, [&](Block* b) {
        if (!b->jac) return fail("%s: a block of level %d has no assembled blocks (registered after the assembly?)", who, level);
        cells += (long)b->v.nx * b->v.ny * b->v.nz;
        return 0;
    });
    if (rc) return rc;
    if (n != cells * g_jac.nState)
        return fail("%s: n=%ld but the matrix of level %d has %ld rows (nState = %d x %ld owned cells)", who, n, level,
                    cells * g_jac.nState, g_jac.nState, cells);
    return 0;
}

int adflow_gpu_jacobian_mult_dev(int level, int transpose, const double* d_x, double* d_y, long n)
{
    if (jm_check(level, d_x, d_y, n)) return 1;
    if (jm_mult_enqueue(level, transpose, d_x, d_y)) return 1;
    return sync_and_check();
}

int adflow_gpu_jacobian_mult(int level, int transpose, const double* x, double* y, long n)
{
    Stage s;
    return jm_check(level, x, y, n) || stage_open(&s, n, 2) || s.in(0, x) || jm_mult_enqueue(level, transpose, s[0], s[1]) ||
           s.out(y, 1) || s.done();
}

// ---- several vectors at once: the product, the ILU application and GMRES on nvec columns that lie ld doubles apart ---------------
// What every multi entry checks of its two sets of columns: nvec, the leading dimensions and that no column of the one set shares
// memory with a column of the other (column a of `in` with column b of `out` included).  `who` is the entry
static_assert(GM_MAXV == ADFLOW_GPU_MAX_NVEC, "GmCoef of kernels_pc.hip holds a coefficient for every column of a call");
static int multi_check(const char* who, int nvec, const double* in, long ldin, const double* out, long ldout, long n)
{
    if (nvec < 1 || nvec > ADFLOW_GPU_MAX_NVEC)
        return fail("%s: nvec = %d; one call takes 1 to %d columns", who, nvec, ADFLOW_GPU_MAX_NVEC);
    if (n < 0 || ldin < n || ldout < n)
        return fail("%s: leading dimensions %ld and %ld, but a column holds n = %ld entries (ld >= n)", who, ldin, ldout, n);
    if (!in || !out) return 0;        // the entry's own check names the NULL
    const uintptr_t pi = (uintptr_t)in, po = (uintptr_t)out, len = (uintptr_t)n * sizeof(double);
    for (int a = 0; a < nvec; ++a)
        for (int b = 0; b < nvec; ++b) {
            const uintptr_t ia = pi + (uintptr_t)a * ldin * sizeof(double), ob = po + (uintptr_t)b * ldout * sizeof(double);
            if (ia < ob + len && ob < ia + len)
                return fail("%s: column %d of the input and column %d of the result overlap (not done in place)", who, a, b);
        }
    return 0;
}

// A host form with columns: set q of nvec columns side by side (ld = n) in the staging area, column c at s[q nvec + c]
static int stage_in_columns(const Stage& s, int q0, const double* h, long ld, int nvec)
{
    for (int c = 0; c < nvec; ++c)
        if (s.in(q0 + c, h + c * ld)) return 1;
    return 0;
}
static int stage_out_columns(const Stage& s, double* h, long ld, int q0, int nvec)
{
    for (int c = 0; c < nvec; ++c)
        if (s.out(h + c * ld, q0 + c)) return 1;
    return 0;
}

// the columns in groups of at most JM_MAXW, each group one pass over the matrix; one column is the product it always was
static int jm_mult_multi_enqueue(int level, int transpose, int nvec, const double* d_x, long ldx, double* d_y, long ldy)
{
    for (int c = 0; c < nvec; c += JM_MAXW)
        if (jm_mult_enqueue(level, transpose, d_x + c * ldx, d_y + c * ldy, std::min<int>(JM_MAXW, nvec - c), ldx, ldy)) return 1;
    return 0;
}

int adflow_gpu_jacobian_mult_multi_dev(int level, int transpose, int nvec, const double* d_X, long ldx, double* d_Y, long ldy, long n)
{
    if (multi_check("jacobian_mult_multi", nvec, d_X, ldx, d_Y, ldy, n) || jm_check(level, d_X, d_Y, n, "jacobian_mult_multi")) return 1;
    if (jm_mult_multi_enqueue(level, transpose, nvec, d_X, ldx, d_Y, ldy)) return 1;
    return sync_and_check();
}

int adflow_gpu_jacobian_mult_multi(int level, int transpose, int nvec, const double* X, long ldx, double* Y, long ldy, long n)
{
    Stage s;
    return multi_check("jacobian_mult_multi", nvec, X, ldx, Y, ldy, n) || jm_check(level, X, Y, n, "jacobian_mult_multi") ||
           stage_open(&s, n, 2 * nvec) || stage_in_columns(s, 0, X, ldx, nvec) ||
           jm_mult_multi_enqueue(level, transpose, nvec, s[0], n, s[nvec], n) || stage_out_columns(s, Y, ldy, nvec, nvec) || s.done();
}

// ---- block ILU(0) of the 7-point preconditioner matrix and right-preconditioned GMRES (kernels_pc.hip) --------------------------
// The PCApply and the KSPSolve of setupStandardKSP (adjointUtils.F90:1374-1562) in the configuration PCBJACOBI / ILU(0) / natural
// ordering, one subdomain per block; see the header for what is out of scope.
namespace {
// adflow_gpu_pc_set_its: the Richardson iterations around the factor (globalPreConIts, localPreConIts and amgLocalPreConIts below level 1)
struct PcIts {
    int outer = 1, inner = 1, innerCoarse = 1;
    bool operator==(const PcIts& o) const { return outer == o.outer && inner == o.inner && innerCoarse == o.innerCoarse; }
};
// What the iterations of a factor need beyond the factor (kernels_pc_rich.hip): the copy of the 7-point matrix of the whole level as
// it stood at the setup, its tables and the work vectors of the recurrences.  Everything is allocated through pc_alloc of the factor
// that owns it, so pc_info counts it and pc_release frees it.
struct PcRich {
    PcRichTab tab;
    size_t matBytes = 0;              // the copy and its tables
    int nWork = 0, width = 1;         // work vectors per column (0, 2 or 4) and the columns they serve at once (pc_ws_reserve)
    double* work = nullptr;           // nWork x width vectors; vector q of column v at work + (q width + v) n
};
struct PcFactor {
    bool valid = false;
    PcIts its;                        // what the factor was built with
    PcRich* rich = nullptr;           // its.outer > 1, or its.inner > 1 on a plain factor (owned)
    int level = 0, nState = 0, nPlanes = 0;      // nPlanes: hyperplanes at fill 0, dependency level sets at fill 1 and 2
    int fill = 0, nEnt = 7;                        // levels of fill the factor was built with and its entries per row
    int coupled = 0;                  // adflow_gpu_pc_set_coupled: 1 = one subdomain for the level (kernels_pc_coupled.hip)
    long nCross = 0;                  // entries of M whose column lies behind a block interface (coupled only)
    long ncell = 0;
    int wsWidth = 1;                  // vectors the work space serves at once: tab.ws, and tab.wsx for the others (pc_ws_reserve)
    size_t bytes = 0;
    std::vector<void*> raw;
    std::vector<int> planeStart;      // first position of every hyperplane in the order of the factor, and the end
    PcTab tab;
    struct PcMg* mg = nullptr;        // adflow_gpu_pc_set_mg with levels > 1: the hierarchy this factor is level 1 of (owned)
    struct PcLevel* lvl = nullptr;    // adflow_gpu_pc_set_level_fill >= 0: the tables of the general pattern (owned); tab is not used then
};
// The ILU(k) over the whole level on a general block pattern (kernels_pc_level.hip): its tables hang on the pattern, not on the numbers,
// and outlive a new setup of the same level and fill on the same blocks and comm pattern (ANKStep sets up at every Jacobian refresh).
struct PcLevel {
    PclTab tab;
    long gen = -1;                    // g_pc_topo_gen the tables were built at
    int maxRow = 0, reused = 0;       // the longest row; 1: the last setup kept the tables and redid the numbers only
    long nEntries = 0;                // blocks of the pattern over all rows, diagonal included
    std::vector<int> vec, cblk;       // host copies for the message of a failing pivot
    int order = 0;                    // adflow_gpu_pc_set_ordering the tables were built with
    long permGen = 0;                 // order 2: g_pc_order_gen of the slot when the tables were built
    long bandwidth = 0;               // max |ordered(column) - ordered(row)| over the assembled entries
    std::vector<int> perm;            // order != 0: perm[new] = old the tables were built with
    JmBlk* dblk = nullptr;            // the block table on the device (the assembly may have moved: written at every setup)
};
// The multigrid hierarchy of a slot (kernels_pc_mg.hip).  Level 1 is lv[0]: its matrix is the slot's own copy of the in-block 7-point
// blocks (T included) and its factor is the PcFactor that owns this hierarchy; the levels below carry their own factor.
struct PcMgLevel {
    std::vector<JmBlk> hb;            // the blocks of the level in its own box layout: jac = its matrix, vecOff = first cell
    JmBlk* dtab = nullptr;            // the same on the device
    long ncell = 0;
    int maxnx = 0, maxny = 0, maxnz = 0;
    double* v[4] = {nullptr, nullptr, nullptr, nullptr};      // rhs, sol, res, x of the cycle
    double* w[2] = {nullptr, nullptr};                        // inner iterations > 1 on this level: their residual, their result
    PcFactor fac;                     // levels >= 2
};
struct PcMg {
    int nSmooth = 1, fillCoarse = 0;
    PcMgSten sten;
    std::vector<int> nnOf;            // block number of every slot of the tables
    std::vector<PcMgLevel> lv;
    std::vector<void*> raw;           // matrices, vectors and tables of the levels (the factors own theirs)
    size_t bytes = 0;
};
struct PcMgSetting { int levels = 1, nSmooth = 1, fillCoarse = 0; };
PcMgSetting g_pc_mg[2];              // adflow_gpu_pc_set_mg: what the next setup of each slot builds (outlives the factors)
PcFactor g_pc_slots[2];              // adflow_gpu_pc_select: e.g. the flow factor and the turbulence factor of ANK_jacobianLag
int g_pc_slot = 0;
int g_pc_fill[2] = {0, 0};           // adflow_gpu_pc_set_fill: the fill the next setup of each slot uses (outlives the factors)
int g_pc_coupled[2] = {0, 0};        // adflow_gpu_pc_set_coupled: 1 = the next setup of the slot factors the whole level as one subdomain
int g_pc_level_fill[2] = {-1, -1};   // adflow_gpu_pc_set_level_fill: >= 0 = the next setup of the slot builds the ILU(fill) of the whole level
int g_pc_order[2] = {0, 0};          // adflow_gpu_pc_set_ordering: 0 natural, 1 RCM, 2 the permutation below (outlives the factors)
std::vector<int> g_pc_order_perm[2]; // adflow_gpu_pc_set_ordering_perm: perm[new] = old, empty = none stored
long g_pc_order_gen[2] = {0, 0};     // counts the calls of adflow_gpu_pc_set_ordering_perm: tables built before the last one are not kept
PcIts g_pc_its[2];                   // adflow_gpu_pc_set_its: the iterations the next setup of each slot builds (outlives the factors)
static PcFactor& pc_sel() { return g_pc_slots[g_pc_slot]; }
struct DevBuf {                       // a device allocation that lives as long as one call
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
}  // namespace

// everything the factor holds, the hierarchy below it included
static size_t pc_bytes(const PcFactor& f)
{
    size_t n = f.bytes;
    if (f.mg) {
        n += f.mg->bytes;
        for (const PcMgLevel& l : f.mg->lv) n += l.fac.bytes;
    }
    return n;
}

static int64_t pc_release(PcFactor& f)
{
    const int64_t n = (int64_t)pc_bytes(f);
    if (f.mg) {
        for (PcMgLevel& l : f.mg->lv)
            for (void* p : l.fac.raw) (void)hipFree(p);
        for (void* p : f.mg->raw) (void)hipFree(p);
        delete f.mg;
    }
    for (void* p : f.raw) (void)hipFree(p);
    delete f.lvl;
    delete f.rich;
    f = PcFactor();
    return n;
}

static int64_t pc_release_all()
{
    int64_t n = 0;
    for (PcFactor& f : g_pc_slots) n += pc_release(f);
    return n;
}

int adflow_gpu_pc_select(int slot)
{
    if (slot < 0 || slot > 1) return fail("pc_select: slot %d; the library keeps two factors, slot 0 and slot 1", slot);
    g_pc_slot = slot;
    return 0;
}

// device memory of the factor f, which is being built with `fill` levels of fill
static int pc_alloc(PcFactor& f, int fill, void** p, size_t bytes)
{
    *p = nullptr;
    if (hipMalloc(p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return fail("pc_setup: cannot allocate %zu bytes (%.1f MB) for the factor of fill %d; %zu bytes of it are held, no factor is "
                    "kept", bytes, bytes / 1048576.0, fill, f.bytes);
    }
    f.raw.push_back(*p);
    f.bytes += bytes;
    return 0;
}

// ---- fill 1 and 2 (kernels_pc_fill.hip) ---------------------------------------------------------------------------------------
// The level-of-fill pattern of a 7-point stencil in the natural ordering, in offset space: level(d) = min over a lower offset a and an
// upper offset b with a + b = d of level(a) + level(b) + 1, kept while <= fill (the symbolic ILU(k) of an unbounded grid; inside a
// block the pattern is this stencil cut at the faces for fill <= 2).  off[]: the offsets (di, dj, dk) in ascending column order,
// lower entries first, the diagonal in the middle.  Returns the number of entries.
static int pc_fill_offsets(int fill, std::vector<std::array<int, 3>>& off)
{
    typedef std::array<int, 3> O;                  // (dk, dj, di): compares as the natural ordering does
    std::map<O, int> lev;
    lev[O{0, 0, 0}] = 0;
    for (int a = 0; a < 3; ++a)
        for (int sg = -1; sg <= 1; sg += 2) {
            O o{0, 0, 0};
            o[a] = sg;
            lev[o] = 0;
        }
    const O zero{0, 0, 0};
    for (bool changed = true; changed;) {
        changed = false;
        const std::map<O, int> was = lev;
        for (auto& lo : was)
            for (auto& up : was) {
                if (!(lo.first < zero) || !(zero < up.first)) continue;
                const O d{lo.first[0] + up.first[0], lo.first[1] + up.first[1], lo.first[2] + up.first[2]};
                const int l = lo.second + up.second + 1;
                if (l > fill) continue;
                auto it = lev.find(d);
                if (it == lev.end() || l < it->second) { lev[d] = l; changed = true; }
            }
    }
    off.clear();
    for (auto& kv : lev) off.push_back({kv.first[2], kv.first[1], kv.first[0]});
    return (int)off.size();
}

// fill 1 and 2: the off-diagonal slots in the order of kernels_pc_fill.hip (the pattern in ascending column order without the diagonal),
// and into T the stencil entry of the assembly every slot starts from and the slot every product L U lands in
static int pc_fill_tables(int fill, const int* sten7, PcTab& T, std::vector<std::array<int, 3>>& slots)
{
    std::vector<std::array<int, 3>> off;
    const int nEnt = pc_fill_offsets(fill, off), nLow = (nEnt - 1) / 2;
    if (nEnt != (fill == 1 ? 13 : 23)) return fail("pc_setup: internal: the pattern of fill %d has %d offsets", fill, nEnt);
    // slot of an entry: lower entries 0..nLow-1, upper entries nLow..2 nLow-1 (both ascending), the diagonal 2 nLow
    auto slotOf = [&](int e) { return e < nLow ? e : e == nLow ? 2 * nLow : e - 1; };
    auto find = [&](int di, int dj, int dk) {
        for (int e = 0; e < nEnt; ++e)
            if (off[e][0] == di && off[e][1] == dj && off[e][2] == dk) return e;
        return -1;
    };
    for (int e = 0; e < nEnt; ++e) {
        const auto& o = off[e];
        const int nz = (o[0] != 0) + (o[1] != 0) + (o[2] != 0);
        int a = -1;
        if (nz == 0) a = sten7[6];
        for (int ax = 0; ax < 3; ++ax)
            if (nz == 1 && o[ax] == -1) a = sten7[ax];          // the column c - e_ax
            else if (nz == 1 && o[ax] == 1) a = sten7[3 + ax];
        T.asmEnt[slotOf(e)] = a;
    }
    for (int e = 0; e < nLow; ++e)
        for (int u = 0; u < nLow; ++u) {
            const auto &a = off[e], &b = off[nLow + 1 + u];
            const int t = find(a[0] + b[0], a[1] + b[1], a[2] + b[2]);
            T.tgt[e * nLow + u] = (signed char)(t < 0 ? -1 : slotOf(t));
        }
    slots = off;
    slots.erase(slots.begin() + nLow);
    return 0;
}

// The tables of the factor f at any fill, its factorisation and its fields.  The caller has filled ncell, sten, asmEnt and tgt of
// f.tab; slots[s] = the offset (di, dj, dk) of the column of off-diagonal slot s, the lower entries in the first half, in the order
// the kernels of this fill number their slots (PcTab, internal.h): nothing is sorted here.  The order of the factor is (set, block, k,
// j, i), set = 1 + the highest set of a lower entry inside the block (longest path; the natural order visits the lower entries of a
// row before the row) -- for the 7-point pattern of fill 0 that is i + j + k, the hyperplanes, and fill 0 takes it and its six
// neighbours directly: the tables are those of the generic loops, which cost its table build a third more time.
// shift != NULL: the pseudo-time term of ANK (tsm of kernels_ank.hip) is added to the diagonal blocks as the factorisation reads them
// mgLevel > 0: hb are the blocks of that level of a multigrid hierarchy (their own box layout and matrix), named in the message
// ccol != NULL (fill 0 only): one subdomain for the level (kernels_pc_coupled.hip).  ccol[d N + c] is the natural number of the column
// of slot d of cell c in whichever block it lies (pc_coupled_columns), -1: none.  A neighbour is lower when its number is smaller;
// the sets are the longest path over the lower neighbours of the whole level, and the word of every cell (PcTab::cw) goes with nbr[].
static int pc_build(PcFactor& f, int level, int fill, const std::vector<std::array<int, 3>>& slots, const std::vector<JmBlk>& hb,
                    const std::vector<int>& nnOf, const double* shift, double turbDiag, int mgLevel = 0,
                    const std::vector<int>* ccol = nullptr)
{
    const int nS = g_jac.nState, nOff = (int)slots.size(), nLow = nOff / 2, nEnt = nOff + 1;
    PcTab& T = f.tab;
    const long N = T.ncell;
    // the natural number of the column of slot e of the cell (i, j, k), number nat, of block q; -1 outside the block
    auto column = [&](const JmBlk& q, long nat, int i, int j, int k, int e) -> long {
        const int di = slots[e][0], dj = slots[e][1], dk = slots[e][2];
        if (i + di < 0 || i + di >= q.nx || j + dj < 0 || j + dj >= q.ny || k + dk < 0 || k + dk >= q.nz) return -1;
        return nat + ((long)dk * q.ny + dj) * q.nx + di;
    };
    std::vector<int> lvl(N);
    int nSets = 0;
    for (auto& q : hb) {
        long nat = q.vecOff;
        for (int k = 0; k < q.nz; ++k)
            for (int j = 0; j < q.ny; ++j)
                for (int i = 0; i < q.nx; ++i, ++nat) {
                    int l = i + j + k;            // what the longest path gives at fill 0, without walking it
                    if (ccol) {
                        l = 0;
                        for (int e = 0; e < nOff; ++e) {
                            const long c = (*ccol)[(size_t)e * N + nat];
                            if (c >= 0 && c < nat) l = std::max(l, lvl[c] + 1);
                        }
                    } else if (fill > 0) {
                        l = 0;
                        for (int e = 0; e < nLow; ++e) {
                            const long c = column(q, nat, i, j, k, e);
                            if (c >= 0) l = std::max(l, lvl[c] + 1);
                        }
                    }
                    lvl[nat] = l;
                    nSets = std::max(nSets, l + 1);
                }
    }
    std::vector<int> start(nSets + 1, 0);
    for (long c = 0; c < N; ++c) start[lvl[c] + 1]++;
    for (int p = 0; p < nSets; ++p) start[p + 1] += start[p];
    std::vector<int> cur(start.begin(), start.end() - 1), pos(N), nbr((size_t)nOff * N), vec(N), cblk(N), cbox(N);
    std::vector<unsigned> cw(ccol ? N : 0);
    for (size_t s = 0; s < hb.size(); ++s) {
        const JmBlk& q = hb[s];
        long nat = q.vecOff;
        for (int k = 0; k < q.nz; ++k)
            for (int j = 0; j < q.ny; ++j)
                for (int i = 0; i < q.nx; ++i, ++nat) {
                    const int at = cur[lvl[nat]]++;
                    pos[nat] = at;
                    vec[at] = (int)nat;
                    cblk[at] = (int)s;
                    cbox[at] = (i + 2) + (j + 2) * q.ldi + (k + 2) * q.ldk;
                }
    }
    for (auto& q : hb) {
        long nat = q.vecOff;
        const long sj = q.nx, sk = (long)q.nx * q.ny;
        for (int k = 0; k < q.nz; ++k)
            for (int j = 0; j < q.ny; ++j)
                for (int i = 0; i < q.nx; ++i, ++nat) {
                    const long at = pos[nat];
                    if (ccol) {
                        unsigned w = 0;
                        for (int e = 0; e < nOff; ++e) {
                            const long c = (*ccol)[(size_t)e * N + nat];
                            nbr[(size_t)e * N + at] = c >= 0 ? pos[c] : -1;
                            if (c < 0) continue;
                            if (c < nat) w |= 1u << e;
                            // the way back: the opposite direction inside a block, any across an interface (pc_coupled_columns has
                            // checked that there is exactly one)
                            int b = (e + 3) % 6, tries = 0;
                            while ((*ccol)[(size_t)b * N + c] != nat && ++tries < 6) b = (b + 1) % 6;
                            if (tries == 6) return fail("pc_setup: internal: a column of the level does not lead back to its row");
                            w |= (unsigned)b << (6 + 3 * e);
                        }
                        cw[at] = w;
                        continue;
                    }
                    if (fill == 0) {              // the six neighbours directly (-i, -j, -k, +i, +j, +k): the generic loop below
                        nbr[0 * N + at] = i > 0 ? pos[nat - 1] : -1;      // gives the same table a third slower
                        nbr[1 * N + at] = j > 0 ? pos[nat - sj] : -1;
                        nbr[2 * N + at] = k > 0 ? pos[nat - sk] : -1;
                        nbr[3 * N + at] = i < q.nx - 1 ? pos[nat + 1] : -1;
                        nbr[4 * N + at] = j < q.ny - 1 ? pos[nat + sj] : -1;
                        nbr[5 * N + at] = k < q.nz - 1 ? pos[nat + sk] : -1;
                        continue;
                    }
                    for (int e = 0; e < nOff; ++e) {
                        const long c = column(q, nat, i, j, k, e);
                        nbr[(size_t)e * N + at] = c >= 0 ? pos[c] : -1;
                    }
                }
    }
    void *dn, *dv, *db, *dc, *dt, *df, *dw = nullptr;
    auto alloc = [&](void** p, size_t bytes) { return pc_alloc(f, fill, p, bytes); };
    if (ccol) {
        if (alloc(&dw, sizeof(unsigned) * N)) return 1;
        HIPCHK(hipMemcpy(dw, cw.data(), sizeof(unsigned) * N, hipMemcpyHostToDevice));
    }
    T.cw = (const unsigned*)dw;
    if (alloc((void**)&T.fac, (size_t)N * nEnt * nS * nS * sizeof(double))) return 1;
    if (alloc((void**)&T.ws, (size_t)N * nS * sizeof(double))) return 1;
    if (alloc(&dn, sizeof(int) * nbr.size()) || alloc(&dv, sizeof(int) * N) || alloc(&db, sizeof(int) * N) || alloc(&dc, sizeof(int) * N) ||
        alloc(&dt, sizeof(JmBlk) * hb.size()) || alloc(&df, sizeof(int)))
        return 1;
    HIPCHK(hipMemcpy(dn, nbr.data(), sizeof(int) * nbr.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv, vec.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, cblk.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dc, cbox.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dt, hb.data(), sizeof(JmBlk) * hb.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(df, 0, sizeof(int), g_stream));
    T.nbr = (const int*)dn; T.vec = (const int*)dv; T.cblk = (const int*)db; T.cbox = (const int*)dc;
    T.blk = (const JmBlk*)dt; T.flag = (int*)df;
    T.tsm = shift; T.turbDiag = turbDiag;
    const int rcf = ccol ? launch_pcc_factor(T, nS, start, g_stream)
                  : fill > 0 ? launch_pcf_factor(T, nS, nEnt, start, g_stream) : launch_pc_factor(T, nS, start, g_stream);
    T.tsm = nullptr;                              // the sweeps do not read it, and it may be released before the factor
    if (rcf) return 1;
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, df, sizeof(int), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    HIPCHK(hipGetLastError());
    if (flag) {
        const int at = flag - 1, s = cblk[at];
        const long loc = vec[at] - hb[s].vecOff;
        if (mgLevel > 0)
            return fail("pc_setup: the pivot block of cell (%d,%d,%d) of block %d on multigrid level %d is singular or not finite (ILU(%d) "
                        "in natural order, level %d); nothing is kept", (int)(loc % hb[s].nx) + 2, (int)(loc / hb[s].nx % hb[s].ny) + 2,
                        (int)(loc / ((long)hb[s].nx * hb[s].ny)) + 2, nnOf[s], mgLevel, fill, level);
        return fail("pc_setup: the pivot block of cell (%d,%d,%d) of block %d is singular or not finite (ILU(%d) in natural order, "
                    "level %d); no factor is kept", (int)(loc % hb[s].nx) + 2, (int)(loc / hb[s].nx % hb[s].ny) + 2,
                    (int)(loc / ((long)hb[s].nx * hb[s].ny)) + 2, nnOf[s], fill, level);
    }
    f.level = level; f.nState = nS; f.nPlanes = nSets; f.ncell = N;
    f.fill = fill; f.nEnt = nEnt;
    f.coupled = ccol ? 1 : 0;
    f.planeStart = start;
    f.valid = true;
    return 0;
}

// the seven points of the assembled stencil in the order of PcTab::sten and the blocks of `level` as the factor kernels see the
// assembly (vecOff: the first CELL of the block in the PETSc layout); N: the owned cells of the level
static int pc_level_blocks(int level, int* sten, std::vector<JmBlk>& hb, std::vector<int>& nnOf, long& N)
{
    const int nS = g_jac.nState;
    for (int q = 0; q < 7; ++q) sten[q] = -1;
    for (int s = 0; s < g_jac.nStencil; ++s) {
        const int* d = g_jac.st[s];               // the column of entry s is the row cell - d
        const int nz = (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
        if (nz == 0) sten[6] = s;
        for (int a = 0; a < 3; ++a)
            if (nz == 1 && d[a] == 1) sten[a] = s;
            else if (nz == 1 && d[a] == -1) sten[3 + a] = s;
    }
    for (int q = 0; q < 7; ++q)
        if (sten[q] < 0) return fail("pc_setup: the assembled stencil lacks one of the seven points");
    std::map<int, Block*> byNN;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level) byNN[std::get<2>(kv.first)] = kv.second;
    if (byNN.empty()) return fail("no block registered on level %d", level);
    N = 0;
    for (auto& kv : byNN) {
        Block* b = kv.second;
        const BlkView& v = b->v;
        if (!b->jac || b->jac_ncomp != 7 * nS * nS)
            return fail("pc_setup: a block of level %d has no assembled blocks (registered after the assembly?)", level);
        if ((double)v.nbox * nS * nS * 8.0 >= 4294967296.0)
            return fail("pc_setup: block of %ld box cells: nState^2 planes exceed the 4 GiB the kernels address from one base", v.nbox);
        JmBlk q;
        memset(&q, 0, sizeof q);
        q.nx = v.nx; q.ny = v.ny; q.nz = v.nz; q.il = v.il; q.jl = v.jl; q.kl = v.kl; q.ib = v.ib; q.jb = v.jb; q.kb = v.kb;
        q.ldi = v.ldi; q.ldk = v.ldk; q.nbox = v.nbox;
        q.jac = b->jac;
        q.vecOff = N;                             // here: the first CELL of the block in the PETSc layout
        hb.push_back(q);
        nnOf.push_back(kv.first);
        N += (long)v.nx * v.ny * v.nz;
    }
    if ((double)N * nS * 8.0 >= 4294967296.0)
        return fail("pc_setup: %ld cells on level %d: a vector of the factor exceeds the 4 GiB the kernels address from one base", N, level);
    // (the factor itself may exceed 4 GiB at any fill: its component planes are reached by 64-bit pointer arithmetic, and the 32-bit
    // byte offset spans the N positions of one plane, which the check above covers)
    return 0;
}

// the table of f for N cells at `fill` and the offsets of its off-diagonal slots: what pc_build expects to find
static int pc_tab_init(PcFactor& f, int fill, long N, const int* sten, std::vector<std::array<int, 3>>& slots)
{
    PcTab& T = f.tab;
    memset(&T, 0, sizeof T);
    T.ncell = N;
    for (int q = 0; q < 7; ++q) T.sten[q] = sten[q];
    // fill 0 (kernels_pc.hip): the slots -i, -j, -k, +i, +j, +k; asmEnt and tgt stay zero
    slots = {{-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (fill > 0 && pc_fill_tables(fill, sten, T, slots)) return 1;
    return 0;
}

// One subdomain for the level (adflow_gpu_pc_set_coupled): col[d N + c] = the natural number (PETSc layout: block after block in
// ascending nn, then k, j, i) of the column of cell c in direction d (0..2: -i, -j, -k; 3..5: +i, +j, +k), -1: none.  Inside a block
// the neighbour; on a first-layer face halo the owned cell of this process that the registered 2-layer pattern of the level names as
// its donor (another block, the block itself, any orientation), as adflow_gpu_jacobian_mult reads it; a halo without such a donor
// (boundary faces, halos fed by messages) stays outside M.  nCross: the entries that came from the pattern.  Refused, because the
// per-cell relations of kernels_pc_coupled.hip do not hold: the same column behind two faces of a cell, a cell that is its own
// column, two neighbours of a cell that are neighbours of each other, a neighbour that does not lead back; and a rotational
// periodicity when the matrix covers the velocities, as the product refuses it.
// general: the caller eliminates on a general pattern (pc_level_build), which takes two neighbours that are neighbours of each other
static int pc_coupled_columns(int level, const std::vector<JmBlk>& hb, const std::vector<int>& nnOf, long N, std::vector<int>& col,
                              long& nCross, bool general = false)
{
    col.assign((size_t)6 * N, -1);
    nCross = 0;
    std::vector<char> iface(N, 0);                // cells with a column behind a face: only they can break the relations
    for (auto& q : hb) {
        long nat = q.vecOff;
        const long sj = q.nx, sk = (long)q.nx * q.ny;
        for (int k = 0; k < q.nz; ++k)
            for (int j = 0; j < q.ny; ++j)
                for (int i = 0; i < q.nx; ++i, ++nat) {
                    if (i > 0) col[0 * N + nat] = (int)(nat - 1);
                    if (j > 0) col[1 * N + nat] = (int)(nat - sj);
                    if (k > 0) col[2 * N + nat] = (int)(nat - sk);
                    if (i < q.nx - 1) col[3 * N + nat] = (int)(nat + 1);
                    if (j < q.ny - 1) col[4 * N + nat] = (int)(nat + sj);
                    if (k < q.nz - 1) col[5 * N + nat] = (int)(nat + sk);
                }
    }
    auto it = g_comm.find(std::make_pair(level, 2));
    if (it != g_comm.end()) {
        const CommPattern& cp = it->second;
        if (g_jac.lStart == 0 && g_jac.nState >= 5)
            for (auto& pd : cp.periodic) {
                bool identity = true;
                for (int q = 0; q < 9; ++q)
                    if (pd.rotMatrix[q] != ((q % 4 == 0) ? 1.0 : 0.0)) identity = false;
                if (!identity && !pd.h_block.empty())
                    return fail("pc_setup: rotational periodicity is not supported by the factor over the level (a registered periodic "
                                "transformation of level %d rotates the velocities of its halos); no factor is kept", level);
            }
        std::map<int, int> slotOf;
        for (size_t s = 0; s < nnOf.size(); ++s) slotOf[nnOf[s]] = (int)s;
        const int nc = (int)cp.h_haloBlock.size();
        for (int t = 0; t < nc; ++t) {
            auto hs = slotOf.find(cp.h_haloBlock[t]), ds = slotOf.find(cp.h_donorBlock[t]);
            if (hs == slotOf.end() || ds == slotOf.end()) continue;
            const JmBlk &q = hb[hs->second], &dq = hb[ds->second];
            const int h[3] = {cp.h_haloIdx[t], cp.h_haloIdx[nc + t], cp.h_haloIdx[2 * nc + t]};
            const int g[3] = {cp.h_donorIdx[t] - 2, cp.h_donorIdx[nc + t] - 2, cp.h_donorIdx[2 * nc + t] - 2};
            const int n[3] = {q.nx, q.ny, q.nz};
            // a first-layer FACE halo: one index at 1 or n + 2, the other two owned; it is the column of one owned cell in one direction
            int dir = -1, nOut = 0, c[3];
            for (int a = 0; a < 3; ++a) {
                c[a] = h[a] - 2;
                if (h[a] == 1) { dir = a; c[a] = 0; ++nOut; }
                else if (h[a] == n[a] + 2) { dir = 3 + a; c[a] = n[a] - 1; ++nOut; }
                else if (h[a] < 2 || h[a] > n[a] + 1) nOut += 2;
            }
            if (nOut != 1) continue;
            if (g[0] < 0 || g[0] >= dq.nx || g[1] < 0 || g[1] >= dq.ny || g[2] < 0 || g[2] >= dq.nz) continue;     // no owned cell
            const long nat = q.vecOff + ((long)c[2] * q.ny + c[1]) * q.nx + c[0];
            if (col[(size_t)dir * N + nat] < 0) ++nCross;
            iface[nat] = 1;
            col[(size_t)dir * N + nat] = (int)(dq.vecOff + ((long)g[2] * dq.ny + g[1]) * dq.nx + g[0]);
        }
    }
    // where cell `nat` lies, for the messages: block number and (i, j, k) as the reference counts them
    auto where = [&](long nat, int* ijk) {
        size_t s = 0;
        while (s + 1 < hb.size() && hb[s + 1].vecOff <= nat) ++s;
        const long loc = nat - hb[s].vecOff;
        ijk[0] = (int)(loc % hb[s].nx) + 2; ijk[1] = (int)(loc / hb[s].nx % hb[s].ny) + 2; ijk[2] = (int)(loc / ((long)hb[s].nx * hb[s].ny)) + 2;
        return nnOf[s];
    };
    for (long c = 0; c < N; ++c)
        for (int d = 0; d < 6 && iface[c]; ++d) {
            const long n = col[(size_t)d * N + c];
            if (n < 0) continue;
            int p[3], o[3];
            if (n == c) {
                const int nn = where(c, p);
                return fail("pc_setup: cell (%d,%d,%d) of block %d has itself as a column behind a face (a block periodic onto itself "
                            "over one cell); the factor over the level does not take it, no factor is kept", p[0], p[1], p[2], nn);
            }
            bool back = false;
            for (int e = 0; e < 6; ++e) {
                const long m = col[(size_t)e * N + n];
                if (m == c) back = true;
                if (m < 0 || m == c) continue;
                for (int d2 = 0; d2 < 6 && !general; ++d2)
                    if (d2 != d && col[(size_t)d2 * N + c] == m) {
                        const int nn = where(c, p), nn2 = where(n, o);
                        return fail("pc_setup: two neighbours of cell (%d,%d,%d) of block %d are neighbours of each other (cell (%d,%d,%d) "
                                    "of block %d is one of them: an edge with three blocks around it, or a period of three cells); the "
                                    "factor over the level does not take it, no factor is kept", p[0], p[1], p[2], nn, o[0], o[1], o[2], nn2);
                    }
            }
            for (int d2 = 0; d2 < d; ++d2)
                if (col[(size_t)d2 * N + c] == n) {
                    const int nn = where(c, p);
                    return fail("pc_setup: cell (%d,%d,%d) of block %d has the same column behind two faces (a block periodic onto "
                                "itself over fewer than three cells); the factor over the level does not take it, no factor is kept",
                                p[0], p[1], p[2], nn);
                }
            if (!back) {
                const int nn = where(c, p), nn2 = where(n, o);
                return fail("pc_setup: cell (%d,%d,%d) of block %d has cell (%d,%d,%d) of block %d as a column, which does not have it as "
                            "one (the 2-layer pattern of level %d is not 1-to-1 there); no factor is kept", p[0], p[1], p[2], nn, o[0],
                            o[1], o[2], nn2, level);
            }
        }
    return 0;
}

// ---- the preconditioner Richardson iterations (adflow_gpu_pc_set_its; kernels_pc_rich.hip) ----------------------------------------
// What the host decides before anything is allocated: the blocks of the assembly, the column table of the whole level
// (pc_coupled_columns in its general mode, with its refusals) and the word of every row -- which columns lie behind a block face, and
// in which direction every column keeps its entry back to the row (the mirror entry of the transposed product).
namespace {
struct PcRichHost {
    int sten[7];
    std::vector<JmBlk> hb;
    long N = 0;
    std::vector<int> col;
    std::vector<unsigned> cw;
};
}  // namespace

static int pc_rich_tables(int level, PcRichHost& H)
{
    std::vector<int> nnOf;
    long nCross = 0;
    if (pc_level_blocks(level, H.sten, H.hb, nnOf, H.N) || pc_coupled_columns(level, H.hb, nnOf, H.N, H.col, nCross, true)) return 1;
    const long N = H.N;
    H.cw.assign(N, 0u);
    for (auto& q : H.hb) {
        long nat = q.vecOff;
        for (int k = 0; k < q.nz; ++k)
            for (int j = 0; j < q.ny; ++j)
                for (int i = 0; i < q.nx; ++i, ++nat) {
                    const bool inside[6] = {i > 0, j > 0, k > 0, i < q.nx - 1, j < q.ny - 1, k < q.nz - 1};
                    unsigned w = 0;
                    for (int d = 0; d < 6; ++d) {
                        const long n = H.col[(size_t)d * N + nat];
                        if (n < 0) continue;
                        if (!inside[d]) w |= 1u << d;
                        // the way back: the opposite direction inside a block, any across an interface (exactly one: pc_coupled_columns)
                        int b = (d + 3) % 6, tries = 0;
                        while (H.col[(size_t)b * N + n] != nat && ++tries < 6) b = (b + 1) % 6;
                        if (tries == 6) return fail("pc_setup: internal: a column of the level does not lead back to its row");
                        w |= (unsigned)b << (6 + 3 * d);
                    }
                    H.cw[nat] = w;
                }
    }
    return 0;
}

// the numbers of the copy of f from the blocks hb of the assembly as it stands now (T of ANK on the diagonal blocks)
static int pc_rich_copy(PcFactor& f, const std::vector<JmBlk>& hb, const int* sten, const double* shift, double turbDiag)
{
    const int nb = (int)hb.size();
    DevBuf src;
    if (hipMalloc(&src.p, sizeof(JmBlk) * nb) != hipSuccess) {
        (void)hipGetLastError();
        src.p = nullptr;
        return fail("pc_setup: cannot allocate %zu bytes for the block table of the assembly; no factor is kept", sizeof(JmBlk) * nb);
    }
    HIPCHK(hipMemcpy(src.p, hb.data(), sizeof(JmBlk) * nb, hipMemcpyHostToDevice));
    PcMgSten S;
    int maxnx = 0, maxny = 0, maxnz = 0;
    for (int q = 0; q < 7; ++q) S.s[q] = sten[q];
    for (auto& q : hb) { maxnx = std::max(maxnx, q.nx); maxny = std::max(maxny, q.ny); maxnz = std::max(maxnz, q.nz); }
    const PcRichTab& T = f.rich->tab;
    launch_rich_copy((const JmBlk*)src.p, nb, maxnx, maxny, maxnz, g_jac.nState, S, shift, turbDiag, T.ncell, T.col, const_cast<double*>(T.mat),
                     g_stream);
    HIPCHK(hipStreamSynchronize(g_stream));       // the table of the assembly is freed on return
    HIPCHK(hipGetLastError());
    return 0;
}

// The copy, its tables and the work vectors of the factor f, which stands and was built with `its`: outer > 1, or inner > 1 on a
// plain factor.  Work vectors per column: two for the outer loop (its residual, the result of the inner application), two for the
// inner loop of a plain factor (its residual, the correction: no sweep runs in place here).
static int pc_rich_attach(PcFactor& f, const PcIts& its, const PcRichHost& H, const double* shift, double turbDiag)
{
    const int nS = g_jac.nState;
    const long N = H.N;
    PcRich* R = new PcRich;
    f.rich = R;                                   // from here on pc_release(f) frees whatever is held
    memset(&R->tab, 0, sizeof R->tab);
    R->tab.ncell = N;
    R->nWork = (its.outer > 1 ? 2 : 0) + (its.inner > 1 && !f.mg ? 2 : 0);
    const size_t before = f.bytes;
    void *dm, *dc, *dw;
    if (pc_alloc(f, f.fill, &dm, (size_t)7 * nS * nS * N * sizeof(double)) || pc_alloc(f, f.fill, &dc, sizeof(int) * 6 * (size_t)N) ||
        pc_alloc(f, f.fill, &dw, sizeof(unsigned) * (size_t)N))
        return 1;
    R->matBytes = f.bytes - before;
    if (pc_alloc(f, f.fill, (void**)&R->work, (size_t)R->nWork * N * nS * sizeof(double))) return 1;
    HIPCHK(hipMemcpy(dc, H.col.data(), sizeof(int) * 6 * (size_t)N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dw, H.cw.data(), sizeof(unsigned) * (size_t)N, hipMemcpyHostToDevice));
    R->tab.mat = (const double*)dm; R->tab.col = (const int*)dc; R->tab.cw = (const unsigned*)dw;
    return pc_rich_copy(f, H.hb, H.sten, shift, turbDiag);
}

// the factor f of the assembled 7-point matrix of `level` with `fill` levels of fill; coupled: one subdomain for the level (fill 0)
static int pc_setup_build(PcFactor& f, int fill, int coupled, int level, const double* shift, double turbDiag)
{
    int sten[7];
    std::vector<JmBlk> hb;
    std::vector<int> nnOf;
    long N = 0;
    std::vector<std::array<int, 3>> slots;
    if (pc_level_blocks(level, sten, hb, nnOf, N) || pc_tab_init(f, fill, N, sten, slots)) return 1;
    if (!coupled) return pc_build(f, level, fill, slots, hb, nnOf, shift, turbDiag);
    std::vector<int> col;
    long nCross = 0;
    if (pc_coupled_columns(level, hb, nnOf, N, col, nCross) || pc_build(f, level, fill, slots, hb, nnOf, shift, turbDiag, 0, &col))
        return 1;
    f.nCross = nCross;
    return 0;
}

// ---- ILU(k) over the whole level on a general block pattern (adflow_gpu_pc_set_level_fill; kernels_pc_level.hip) ------------------
// The tables of the factor f of `level` at `fill` for the N cells of the blocks hb: the symbolic ILU(fill) of the cell graph of the level
// (columns: pc_coupled_columns), the level sets, the order and the slices of the storage; everything that does not depend on the
// numbers.  The host decides every refusal before the first allocation.
// Ordering (adflow_gpu_pc_set_ordering): everything below the columns runs in the ORDERED numbering a = inv[natural number] -- the
// symbolic factorisation, the ascending columns of a row, the level sets, the order (set, ordered number) of the storage; only vec,
// cblk and cbox lead back to the cell.  order 0: perm and inv stay empty and every number is the natural one, as before.
static int pc_level_tables(PcFactor& f, int level, int fill, const std::vector<JmBlk>& hb, const std::vector<int>& nnOf, long N, int order,
                           const std::vector<int>& callerPerm)
{
    const int nS = g_jac.nState;
    std::vector<int> col;
    long nCross = 0;
    if (pc_coupled_columns(level, hb, nnOf, N, col, nCross, true)) return 1;
    std::vector<int> perm, inv;
    if (order == 1) {
        // the symmetric cell graph of the 7-point pattern, interface columns included, without the diagonal, neighbours ascending
        std::vector<std::vector<int>> nb((size_t)N);
        for (long i = 0; i < N; ++i)
            for (int d = 0; d < 6; ++d) {
                const int c = col[(size_t)d * N + i];
                if (c >= 0 && c != i) {
                    nb[(size_t)i].push_back(c);
                    nb[(size_t)c].push_back((int)i);
                }
            }
        std::vector<size_t> xadj((size_t)N + 1, 0);
        std::vector<int> adj;
        for (long i = 0; i < N; ++i) {
            std::vector<int>& r = nb[(size_t)i];
            std::sort(r.begin(), r.end());
            r.erase(std::unique(r.begin(), r.end()), r.end());
            adj.insert(adj.end(), r.begin(), r.end());
            xadj[(size_t)i + 1] = adj.size();
        }
        pc_order_rcm(N, xadj, adj, perm);
    } else if (order == 2) {
        perm = callerPerm;
    }
    if (order) {
        inv.resize((size_t)N);
        for (long a = 0; a < N; ++a) inv[(size_t)perm[(size_t)a]] = (int)a;
    }
    auto natOf = [&](long a) { return order ? perm[(size_t)a] : (int)a; };
    auto ordOf = [&](int c) { return order ? inv[(size_t)c] : c; };
    long bandwidth = 0;
    // symbolic ILU(fill): level(i, j) = min over the pivots k < min(i, j) of level(i, k) + level(k, j) + 1, kept while <= fill.  One level per
    // entry suffices, the blocks are dense.  Rows in CSR, every row in ascending column order; dg[i]: where the diagonal stands in row i
    std::vector<size_t> rp(N + 1, 0);
    std::vector<int> cj, dg(N);
    std::vector<unsigned char> lv;
    cj.reserve((size_t)N * (fill == 0 ? 7 : fill == 1 ? 14 : fill == 2 ? 26 : 48));
    lv.reserve(cj.capacity());
    std::vector<int> wc;
    std::vector<unsigned char> wl;
    for (long i = 0; i < N; ++i) {
        int a[7], na = 0;
        const long nati = natOf(i);
        for (int d = 0; d < 6; ++d)
            if (col[(size_t)d * N + nati] >= 0) {
                a[na] = ordOf(col[(size_t)d * N + nati]);
                bandwidth = std::max(bandwidth, a[na] > i ? a[na] - i : i - a[na]);
                ++na;
            }
        a[na++] = (int)i;
        std::sort(a, a + na);
        wc.assign(a, a + na);
        wl.assign(na, 0);
        for (size_t p = 0; p < wc.size() && wc[p] < i; ++p) {        // the pivots in ascending order, those the loop adds included
            const int k = wc[p], lk = wl[p];
            if (lk >= fill) continue;                                 // lk + level(k, j) + 1 > fill whatever row k holds
            size_t w = p + 1;
            for (size_t e = rp[k] + dg[k] + 1; e < rp[k + 1]; ++e) { // the upper entries of row k: a merge, both rows ascend
                const int j = cj[e], nw = lk + lv[e] + 1;
                if (nw > fill) continue;
                while (w < wc.size() && wc[w] < j) ++w;
                if (w < wc.size() && wc[w] == j) {
                    if (nw < wl[w]) wl[w] = (unsigned char)nw;
                } else {
                    wc.insert(wc.begin() + w, j);
                    wl.insert(wl.begin() + w, (unsigned char)nw);
                }
            }
        }
        dg[i] = (int)(std::lower_bound(wc.begin(), wc.end(), (int)i) - wc.begin());
        if (wc.size() > 65535)
            return fail("pc_setup: row %ld of the ILU(%d) over level %d has %zu entries; the tables keep the entry number in 16 bits (at most "
                        "65535); no factor is kept", i, fill, level, wc.size());
        cj.insert(cj.end(), wc.begin(), wc.end());
        lv.insert(lv.end(), wl.begin(), wl.end());
        rp[i + 1] = cj.size();
    }
    // level sets: the longest path over the lower entries; the order (set, natural number)
    std::vector<int> lvl(N);
    int nSets = 0, maxRow = 0;
    for (long i = 0; i < N; ++i) {
        int l = 0;
        for (size_t e = rp[i]; e < rp[i] + dg[i]; ++e) l = std::max(l, lvl[cj[e]] + 1);
        lvl[i] = l;
        nSets = std::max(nSets, l + 1);
        maxRow = std::max(maxRow, (int)(rp[i + 1] - rp[i]));
    }
    std::vector<int> start(nSets + 1, 0);
    for (long c = 0; c < N; ++c) start[lvl[c] + 1]++;
    for (int p = 0; p < nSets; ++p) start[p + 1] += start[p];
    // pos: ordered number -> position; ord, vec, cblk, cbox: position -> ordered number, natural number, block slot, box index
    std::vector<int> cur(start.begin(), start.end() - 1), pos(N), ord(N), vec(N), cblk(N), cbox(N);
    for (long a = 0; a < N; ++a) {
        pos[a] = cur[lvl[a]]++;
        ord[pos[a]] = (int)a;
    }
    for (size_t s = 0; s < hb.size(); ++s) {
        const JmBlk& q = hb[s];
        long nat = q.vecOff;
        for (int k = 0; k < q.nz; ++k)
            for (int j = 0; j < q.ny; ++j)
                for (int i = 0; i < q.nx; ++i, ++nat) {
                    const int at = pos[ordOf((int)nat)];
                    vec[at] = (int)nat;
                    cblk[at] = (int)s;
                    cbox[at] = (i + 2) + (j + 2) * q.ldi + (k + 2) * q.ldk;
                }
    }
    // the slices: the rows of one workgroup (64 positions of a set, fewer at its end) share the width of their longest row
    std::vector<long> ebase(N);
    std::vector<int> rinfo(N), rcnt(N);
    long E = 0;
    for (int p = 0; p < nSets; ++p)
        for (int s0 = start[p]; s0 < start[p + 1]; s0 += 64) {
            const int st = std::min(64, start[p + 1] - s0);
            int w = 0;
            for (int t = 0; t < st; ++t) w = std::max(w, (int)(rp[ord[s0 + t] + 1] - rp[ord[s0 + t]]));
            for (int t = 0; t < st; ++t) {
                const int a = ord[s0 + t];
                ebase[s0 + t] = E;
                rinfo[s0 + t] = t | (st << 8);
                rcnt[s0 + t] = dg[a] | ((int)(rp[a + 1] - rp[a]) << 16);
            }
            E += (long)w * st;
        }
    std::vector<int> epos((size_t)E, 0), enat((size_t)E, 0), einfo((size_t)E, 0);
    for (long at = 0; at < N; ++at) {
        const int a = ord[at], nat = vec[at], st = rinfo[at] >> 8, t = rinfo[at] & 0xff;
        for (size_t e = rp[a]; e < rp[a + 1]; ++e) {
            const int c = cj[e];                                       // the ordered number of the column
            const size_t slot = (size_t)ebase[at] + (e - rp[a]) * st + t;
            epos[slot] = pos[c];
            enat[slot] = c;
            int from = 0;                                              // 1 + direction of the assembled entry, 0: a fill entry
            if (c == a) from = 7;
            else if (lv[e] == 0)
                for (int d = 0; d < 6; ++d)
                    if (col[(size_t)d * N + nat] == natOf(c)) from = d + 1;
            const int* rb = cj.data() + rp[c];
            const int* re = cj.data() + rp[c + 1];
            const int* mi = std::lower_bound(rb, re, a);
            if (mi == re || *mi != a)
                return fail("pc_setup: the pattern of the ILU(%d) over level %d has the entry (%d, %d) but not its mirror entry: a column that "
                            "does not lead back; no factor is kept", fill, level, nat, natOf(c));
            einfo[slot] = (int)(mi - rb) | (from << 16);
        }
    }
    // ---- device: the factor, its work space, the tables
    PcLevel* L = new PcLevel;
    f.lvl = L;                                    // from here on pc_release(f) frees whatever is held
    memset(&f.tab, 0, sizeof f.tab);
    memset(&L->tab, 0, sizeof L->tab);
    f.tab.ncell = N;
    PclTab& T = L->tab;
    T.ncell = N;
    void *de, *dr, *dc, *dp, *dn, *di, *dv, *db, *dx, *df;
    auto alloc = [&](void** p, size_t bytes) { return pc_alloc(f, fill, p, bytes); };
    if (alloc((void**)&T.fac, (size_t)E * nS * nS * sizeof(double)) || alloc((void**)&f.tab.ws, (size_t)N * nS * sizeof(double)) ||
        alloc((void**)&T.rpiv, sizeof(int) * N))
        return 1;
    if (alloc(&de, sizeof(long) * N) || alloc(&dr, sizeof(int) * N) || alloc(&dc, sizeof(int) * N) || alloc(&dp, sizeof(int) * (size_t)E) ||
        alloc(&dn, sizeof(int) * (size_t)E) || alloc(&di, sizeof(int) * (size_t)E) || alloc(&dv, sizeof(int) * N) ||
        alloc(&db, sizeof(int) * N) || alloc(&dx, sizeof(int) * N) || alloc((void**)&L->dblk, sizeof(JmBlk) * hb.size()) ||
        alloc(&df, sizeof(int)))
        return 1;
    // (padding slots of the factor are never read; cleared so that a download of the storage shows no stale numbers)
    HIPCHK(hipMemsetAsync(T.fac, 0, (size_t)E * nS * nS * sizeof(double), g_stream));
    HIPCHK(hipMemcpy(de, ebase.data(), sizeof(long) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dr, rinfo.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dc, rcnt.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dp, epos.data(), sizeof(int) * (size_t)E, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dn, enat.data(), sizeof(int) * (size_t)E, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(di, einfo.data(), sizeof(int) * (size_t)E, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dv, vec.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, cblk.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dx, cbox.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    T.ws = f.tab.ws;
    T.ebase = (const long*)de; T.rinfo = (const int*)dr; T.rcnt = (const int*)dc;
    T.epos = (const int*)dp; T.enat = (const int*)dn; T.einfo = (const int*)di;
    T.vec = (const int*)dv; T.cblk = (const int*)db; T.cbox = (const int*)dx;
    T.blk = L->dblk; T.flag = (int*)df;
    L->gen = g_pc_topo_gen;
    L->maxRow = maxRow;
    L->nEntries = (long)cj.size();
    L->vec = vec;
    L->cblk = cblk;
    L->order = order;
    L->permGen = g_pc_order_gen[g_pc_slot];
    L->bandwidth = bandwidth;
    L->perm.swap(perm);
    f.level = level; f.nState = nS; f.nPlanes = nSets; f.ncell = N;
    f.fill = fill; f.nEnt = maxRow;
    f.coupled = 1;
    f.nCross = nCross;
    f.planeStart = start;
    return 0;
}

// the numbers of the factor over the level f, whose tables stand: the assembled rows into its storage, the elimination, the pivots
static int pc_level_numeric(PcFactor& f, const int* sten, const std::vector<JmBlk>& hb, const std::vector<int>& nnOf, const double* shift,
                            double turbDiag)
{
    PcLevel& L = *f.lvl;
    PclTab T = L.tab;
    for (int q = 0; q < 7; ++q) T.sten[q] = sten[q];
    T.tsm = shift; T.turbDiag = turbDiag;
    HIPCHK(hipMemcpyAsync(L.dblk, hb.data(), sizeof(JmBlk) * hb.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemsetAsync(T.flag, 0, sizeof(int), g_stream));
    if (launch_pcl_factor(T, f.nState, f.planeStart, g_stream)) return 1;
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, T.flag, sizeof(int), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));       // hb, which the copy above reads, lives until the caller returns
    HIPCHK(hipGetLastError());
    if (flag) {
        const int at = flag - 1, s = L.cblk[at];
        const long loc = L.vec[at] - hb[s].vecOff;
        return fail("pc_setup: the pivot block of cell (%d,%d,%d) of block %d is singular or not finite (ILU(%d) over the level in %s "
                    "order, level %d); no factor is kept", (int)(loc % hb[s].nx) + 2, (int)(loc / hb[s].nx % hb[s].ny) + 2,
                    (int)(loc / ((long)hb[s].nx * hb[s].ny)) + 2, nnOf[s], f.fill,
                    L.order == 0 ? "natural" : L.order == 1 ? "RCM" : "the caller's", f.level);
    }
    f.valid = true;
    return 0;
}

// The ILU(fill) over the whole level in f.  A level factor of the same level, fill and nState that stands in f, built on the blocks and
// comm patterns registered now, keeps its tables (reused = 1); anything else in f is released first.
static int pc_level_setup(PcFactor& f, int fill, int level, const double* shift, double turbDiag)
{
    int sten[7];
    std::vector<JmBlk> hb;
    std::vector<int> nnOf;
    long N = 0;
    const int order = g_pc_order[g_pc_slot];
    const std::vector<int>& perm = g_pc_order_perm[g_pc_slot];
    const bool keep = f.valid && f.lvl && f.level == level && f.fill == fill && f.nState == g_jac.nState && f.lvl->gen == g_pc_topo_gen &&
                      f.lvl->order == order && (order != 2 || f.lvl->permGen == g_pc_order_gen[g_pc_slot]);
    if (!keep) (void)pc_release(f);
    if (pc_level_blocks(level, sten, hb, nnOf, N)) return 1;
    if (keep && N != f.ncell) return fail("pc_setup: internal: the level has %ld cells, the tables of its factor %ld", N, f.ncell);
    if (!keep && order == 2 && perm.empty())
        return fail("pc_setup: slot %d is set to the caller's ordering (adflow_gpu_pc_set_ordering(2)) and holds no permutation: call "
                    "adflow_gpu_pc_set_ordering_perm first; no factor is kept", g_pc_slot);
    if (!keep && order == 2 && (long)perm.size() != N)
        return fail("pc_setup: the permutation of slot %d (adflow_gpu_pc_set_ordering_perm) has %zu entries, level %d has %ld owned cells; "
                    "no factor is kept", g_pc_slot, perm.size(), level, N);
    if (!keep && pc_level_tables(f, level, fill, hb, nnOf, N, order, perm)) return 1;
    f.valid = false;                              // until the numbers stand
    f.lvl->reused = keep ? 1 : 0;
    return pc_level_numeric(f, sten, hb, nnOf, shift, turbDiag);
}

// ---- the multigrid hierarchy (adflow_gpu_pc_set_mg; kernels_pc_mg.hip) -------------------------------------------------------------
// The `mg` preconditioner of amg.F90, block-local like the factor: A_1 = the in-block 7-point matrix (+ T), A_{l+1} = P^T A_l P over
// 2 x 2 x 2 aggregates per block, one block ILU per level (fill of the slot on level 1, fillCoarse below), the cycle of
// amg.F90:712-759.  Every level keeps the blocks in the order of level 1, natural ordering inside a block.
static int pc_mg_alloc(PcMg& M, void** p, size_t bytes, const char* what, int mgLevel)
{
    *p = nullptr;
    if (hipMalloc(p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return fail("pc_setup: cannot allocate %zu bytes (%.1f MB) for the %s of multigrid level %d; nothing is kept", bytes,
                    bytes / 1048576.0, what, mgLevel);
    }
    M.raw.push_back(*p);
    M.bytes += bytes;
    return 0;
}

static int pc_mg_setup_build(PcFactor& f, int fill, const PcMgSetting& set, const PcIts& its, int level, const double* shift, double turbDiag)
{
    const int nS = g_jac.nState;
    int sten[7];
    std::vector<JmBlk> asmb;
    std::vector<int> nnOf;
    long N = 0;
    if (pc_level_blocks(level, sten, asmb, nnOf, N)) return 1;
    PcMg* Mp = new PcMg;
    f.mg = Mp;                                    // from here on pc_release(f) frees whatever the hierarchy holds
    PcMg& M = *Mp;
    M.nSmooth = set.nSmooth; M.fillCoarse = set.fillCoarse; M.nnOf = nnOf;
    for (int q = 0; q < 7; ++q) M.sten.s[q] = sten[q];
    M.lv.resize(set.levels);
    const int nb = (int)asmb.size();
    // the sizes of every level (amg.F90:140-155) and its own box layout: two halo layers, ldi and ldk even
    for (int l = 0; l < set.levels; ++l) {
        PcMgLevel& L = M.lv[l];
        long off = 0;
        for (int s = 0; s < nb; ++s) {
            JmBlk q;
            memset(&q, 0, sizeof q);
            if (l == 0) { q.nx = asmb[s].nx; q.ny = asmb[s].ny; q.nz = asmb[s].nz; }
            else {
                const JmBlk& p = M.lv[l - 1].hb[s];
                q.nx = (p.nx + 1) / 2; q.ny = (p.ny + 1) / 2; q.nz = (p.nz + 1) / 2;
            }
            q.il = q.nx + 1; q.jl = q.ny + 1; q.kl = q.nz + 1; q.ib = q.nx + 3; q.jb = q.ny + 3; q.kb = q.nz + 3;
            q.ldi = (q.nx + 5) & ~1;
            q.ldk = q.ldi * (q.ny + 4);
            q.nbox = (long)q.ldk * (q.nz + 4);
            q.vecOff = off;
            if ((double)q.nbox * nS * nS * 8.0 >= 4294967296.0)
                return fail("pc_setup: block of %ld box cells on multigrid level %d: nState^2 planes exceed the 4 GiB the kernels address "
                            "from one base", q.nbox, l + 1);
            off += (long)q.nx * q.ny * q.nz;
            L.maxnx = std::max(L.maxnx, q.nx); L.maxny = std::max(L.maxny, q.ny); L.maxnz = std::max(L.maxnz, q.nz);
            L.hb.push_back(q);
        }
        L.ncell = off;
        // the coarsening launch carries the nState^2 block components above the j tiles of the coarse level in gridDim.y
        if (l > 0 && (long)((L.maxny + 3) / 4) * nS * nS > 65535)
            return fail("pc_setup: multigrid level %d has a block of %d cells along j: the coarsening launch takes at most %d",
                        l + 1, L.maxny, 4 * (65535 / (nS * nS)));
        if (l > 0 && L.ncell == M.lv[l - 1].ncell)
            return fail("pc_setup: multigrid level %d would have the %ld cells of level %d (every block is 1 x 1 x 1 there): ask for at "
                        "most %d levels; nothing is kept", l + 1, L.ncell, l, l);
    }
    // matrices (zeroed: the halo layers and the second half of a pair past the end of a row are loaded, never used), tables, vectors
    for (int l = 0; l < set.levels; ++l) {
        PcMgLevel& L = M.lv[l];
        size_t nd = 0;
        for (auto& q : L.hb) nd += (size_t)7 * nS * nS * q.nbox;
        double* mat = nullptr;
        if (pc_mg_alloc(M, (void**)&mat, nd * sizeof(double), "matrix", l + 1)) return 1;
        HIPCHK(hipMemsetAsync(mat, 0, nd * sizeof(double), g_stream));
        size_t at = 0;
        for (auto& q : L.hb) {
            q.jac = mat + at;
            at += (size_t)7 * nS * nS * q.nbox;
        }
        if (pc_mg_alloc(M, (void**)&L.dtab, sizeof(JmBlk) * nb, "block table", l + 1)) return 1;
        HIPCHK(hipMemcpy(L.dtab, L.hb.data(), sizeof(JmBlk) * nb, hipMemcpyHostToDevice));
        for (int v = 0; v < 4; ++v)
            if (pc_mg_alloc(M, (void**)&L.v[v], (size_t)L.ncell * nS * sizeof(double), "vectors", l + 1)) return 1;
        // inner iterations on this level (adflow_gpu_pc_set_its): the level owns its matrix, two vectors more is all they need
        for (int v = 0; v < 2 && (l == 0 ? its.inner : its.innerCoarse) > 1; ++v)
            if (pc_mg_alloc(M, (void**)&L.w[v], (size_t)L.ncell * nS * sizeof(double), "vectors of the inner iterations", l + 1)) return 1;
    }
    // level 1: the copy of the in-block blocks with T on the diagonal, then its factor -- of the copy, so without a shift
    {
        DevBuf src;
        if (hipMalloc(&src.p, sizeof(JmBlk) * nb) != hipSuccess) {
            (void)hipGetLastError();
            return fail("pc_setup: cannot allocate %zu bytes for the block table of the assembly; nothing is kept", sizeof(JmBlk) * nb);
        }
        HIPCHK(hipMemcpy(src.p, asmb.data(), sizeof(JmBlk) * nb, hipMemcpyHostToDevice));
        PcMgLevel& L = M.lv[0];
        launch_mg_fine_copy((const JmBlk*)src.p, L.dtab, nb, L.maxnx, L.maxny, L.maxnz, nS, M.sten, shift, turbDiag, N, g_stream);
        HIPCHK(hipStreamSynchronize(g_stream));   // the table of the assembly is freed on return
    }
    std::vector<std::array<int, 3>> slots;
    if (pc_tab_init(f, fill, N, sten, slots) || pc_build(f, level, fill, slots, M.lv[0].hb, nnOf, nullptr, 0.0, 1)) return 1;
    for (int l = 1; l < set.levels; ++l) {
        PcMgLevel &F = M.lv[l - 1], &C = M.lv[l];
        launch_mg_coarsen(F.dtab, C.dtab, nb, C.maxnx, C.maxny, C.maxnz, nS, M.sten, g_stream);
        if (pc_tab_init(C.fac, set.fillCoarse, C.ncell, sten, slots) ||
            pc_build(C.fac, level, set.fillCoarse, slots, C.hb, nnOf, nullptr, 0.0, l + 1))
            return 1;
    }
    return 0;
}

static int pc_setup_check(const char* who, int level)
{
    if (need_ready()) return 1;
    if (!g_jac_valid) return fail("%s: no assembled Jacobian (call adflow_gpu_fd_jacobian with ADFLOW_JAC_PC first)", who);
    if (level != g_jac_level) return fail("%s: level %d is not the level of the assembly (%d)", who, level, g_jac_level);
    if (g_jac.nStencil != 7)
        return fail("%s: the assembled matrix has a %d-point stencil; the block ILU(0) takes the 7-point preconditioner matrix "
                    "(ADFLOW_JAC_PC without ADFLOW_JAC_VISC_PC)", who, g_jac.nStencil);
    return 0;
}

// a new factor in the selected slot at the fill set for that slot; nothing is kept when the build fails
static int pc_setup_selected(int level, const double* shift = nullptr, double turbDiag = 0.0)
{
    PcFactor& f = pc_sel();
    HIPCHK(hipStreamSynchronize(g_stream));
    const PcMgSetting& mg = g_pc_mg[g_pc_slot];
    const int coupled = g_pc_coupled[g_pc_slot];
    const PcIts its = g_pc_its[g_pc_slot];
    PcRichHost H;
    if (g_pc_level_fill[g_pc_slot] >= 0) {
        // the ILU(k) over the level is a factor of its own kind: it takes none of the other settings of the slot
        const int lf = g_pc_level_fill[g_pc_slot];
        const char* with = nullptr;
        char what[96];
        if (coupled) { with = "adflow_gpu_pc_set_coupled"; snprintf(what, sizeof what, "coupled = 1"); }
        else if (g_pc_fill[g_pc_slot] > 0) { with = "adflow_gpu_pc_set_fill"; snprintf(what, sizeof what, "fill %d", g_pc_fill[g_pc_slot]); }
        else if (mg.levels > 1) { with = "adflow_gpu_pc_set_mg"; snprintf(what, sizeof what, "a multigrid hierarchy of %d levels", mg.levels); }
        if (with) {
            (void)pc_release(f);
            return fail("pc_setup: slot %d is set to the ILU(%d) over the level (adflow_gpu_pc_set_level_fill) and to %s (%s); the factor "
                        "over the level takes neither the subdomain setting, nor the block-local fill, nor a hierarchy: set that one back "
                        "or level_fill to -1; no factor is kept", g_pc_slot, lf, what, with);
        }
        // tables that stand are kept only with the iterations they were built for; then the copy is redone, the numbers changed
        if (!(f.its == its)) (void)pc_release(f);
        int rc = pc_level_setup(f, lf, level, shift, turbDiag);
        if (!rc && f.rich) {
            std::vector<int> nnOf;
            rc = pc_level_blocks(level, H.sten, H.hb, nnOf, H.N) || pc_rich_copy(f, H.hb, H.sten, shift, turbDiag);
        } else if (!rc && (its.outer > 1 || its.inner > 1)) {
            rc = pc_rich_tables(level, H) || pc_rich_attach(f, its, H, shift, turbDiag);
        }
        if (rc) {
            if (g_stream) (void)hipStreamSynchronize(g_stream);
            (void)pc_release(f);
            return 1;
        }
        f.its = its;
        return 0;
    }
    (void)pc_release(f);
    if (g_pc_order[g_pc_slot] != 0)
        return fail("pc_setup: slot %d is set to ordering %d (adflow_gpu_pc_set_ordering) without the ILU over the level "
                    "(adflow_gpu_pc_set_level_fill is -1): the patterns of the block-local factors, of coupled = 1 and of a hierarchy are "
                    "fixed stencils of the natural ordering; no factor is kept", g_pc_slot, g_pc_order[g_pc_slot]);
    if (coupled && g_pc_fill[g_pc_slot] > 0)
        return fail("pc_setup: slot %d is set to one subdomain for the level (adflow_gpu_pc_set_coupled) and to fill %d; across a block "
                    "interface the pattern of fill 1 and 2 is no fixed stencil, the factor over the level takes fill 0; no factor is kept",
                    g_pc_slot, g_pc_fill[g_pc_slot]);
    if (coupled && mg.levels > 1)
        return fail("pc_setup: slot %d is set to one subdomain for the level (adflow_gpu_pc_set_coupled) and to a multigrid hierarchy of "
                    "%d levels, which is built block by block; no factor is kept", g_pc_slot, mg.levels);
    // the iterations need the matrix of the whole level: every refusal about its columns before anything is allocated
    const bool copy = its.outer > 1 || (its.inner > 1 && mg.levels <= 1);
    if (copy && pc_rich_tables(level, H)) return 1;
    if ((mg.levels > 1 ? pc_mg_setup_build(f, g_pc_fill[g_pc_slot], mg, its, level, shift, turbDiag)
                       : pc_setup_build(f, g_pc_fill[g_pc_slot], coupled, level, shift, turbDiag)) ||
        (copy && pc_rich_attach(f, its, H, shift, turbDiag))) {
        if (g_stream) (void)hipStreamSynchronize(g_stream);
        (void)pc_release(f);
        return 1;
    }
    f.its = its;
    return 0;
}

int adflow_gpu_pc_setup(int level)
{
    if (pc_setup_check("pc_setup", level)) return 1;
    return pc_setup_selected(level);
}

int adflow_gpu_pc_info(int32_t* nState, int32_t* nPlanes, int64_t* bytes)
{
    if (!pc_sel().valid) return fail("pc_info: no factor (call adflow_gpu_pc_setup first)");
    if (nState) *nState = pc_sel().nState;
    if (nPlanes) *nPlanes = pc_sel().nPlanes;
    if (bytes) *bytes = (int64_t)pc_bytes(pc_sel());
    return 0;
}

int adflow_gpu_pc_info2(int32_t* fill, int32_t* nEntries, int32_t* nLevelSets)
{
    if (!pc_sel().valid) return fail("pc_info2: no factor (call adflow_gpu_pc_setup first)");
    if (fill) *fill = pc_sel().fill;
    if (nEntries) *nEntries = pc_sel().nEnt;
    if (nLevelSets) *nLevelSets = pc_sel().nPlanes;
    return 0;
}

int adflow_gpu_pc_set_fill(int fill)
{
    if (fill < 0 || fill > 2)
        return fail("pc_set_fill: fill %d; the block ILU takes 0, 1 or 2 levels of fill (from 3 on the pattern of a block in the natural "
                    "ordering is no fixed stencil)", fill);
    g_pc_fill[g_pc_slot] = fill;
    return 0;
}

int adflow_gpu_pc_set_coupled(int coupled)
{
    if (coupled != 0 && coupled != 1)
        return fail("pc_set_coupled: %d; 0 = one subdomain per block, 1 = one subdomain for the level", coupled);
    g_pc_coupled[g_pc_slot] = coupled;
    return 0;
}

int adflow_gpu_pc_coupled_info(int32_t* coupled, int32_t* nLevelSets, int64_t* nCrossEntries)
{
    if (!pc_sel().valid) return fail("pc_coupled_info: no factor (call adflow_gpu_pc_setup first)");
    if (coupled) *coupled = pc_sel().coupled;
    if (nLevelSets) *nLevelSets = pc_sel().nPlanes;
    if (nCrossEntries) *nCrossEntries = pc_sel().nCross;
    return 0;
}

int adflow_gpu_pc_set_level_fill(int fill)
{
    if (fill < -1 || fill > 3)
        return fail("pc_set_level_fill: %d; -1 = off, 0, 1, 2 or 3 levels of fill of the ILU over the whole level", fill);
    g_pc_level_fill[g_pc_slot] = fill;
    return 0;
}

int adflow_gpu_pc_level_info(int32_t* fill, int32_t* maxRow, int64_t* nEntries, int32_t* nLevelSets, int64_t* nCrossEntries, int32_t* reused)
{
    const PcFactor& f = pc_sel();
    if (!f.valid) return fail("pc_level_info: no factor (call adflow_gpu_pc_setup first)");
    if (!f.lvl)
        return fail("pc_level_info: the factor of slot %d is no ILU over the level (adflow_gpu_pc_set_level_fill before the setup)", g_pc_slot);
    if (fill) *fill = f.fill;
    if (maxRow) *maxRow = f.lvl->maxRow;
    if (nEntries) *nEntries = f.lvl->nEntries;
    if (nLevelSets) *nLevelSets = f.nPlanes;
    if (nCrossEntries) *nCrossEntries = f.nCross;
    if (reused) *reused = f.lvl->reused;
    return 0;
}

int adflow_gpu_pc_set_ordering(int kind)
{
    if (kind < 0 || kind > 2)
        return fail("pc_set_ordering: %d; 0 = natural, 1 = RCM, 2 = the permutation of adflow_gpu_pc_set_ordering_perm", kind);
    g_pc_order[g_pc_slot] = kind;
    return 0;
}

int adflow_gpu_pc_set_ordering_perm(const int32_t* perm, long n)
{
    if (perm) {
        if (n < 1) return fail("pc_set_ordering_perm: n = %ld; a permutation has at least one entry (index 0); the previous one is kept", n);
        long bad = 0;
        const int rc = pc_order_check_perm(perm, n, &bad);
        if (rc == 1)
            return fail("pc_set_ordering_perm: perm[%ld] = %d lies outside 0 .. %ld; the previous permutation is kept", bad, (int)perm[bad],
                        n - 1);
        if (rc == 2)
            return fail("pc_set_ordering_perm: perm[%ld] = %d occurs twice; the previous permutation is kept", bad, (int)perm[bad]);
        g_pc_order_perm[g_pc_slot].assign(perm, perm + n);
    } else {
        g_pc_order_perm[g_pc_slot].clear();
        g_pc_order_perm[g_pc_slot].shrink_to_fit();
    }
    g_pc_order_gen[g_pc_slot]++;
    return 0;
}

int adflow_gpu_pc_ordering_info(int32_t* kind, int64_t* bandwidth, int32_t* nLevelSets, int64_t* nEntries)
{
    const PcFactor& f = pc_sel();
    if (!f.valid) return fail("pc_ordering_info: no factor (call adflow_gpu_pc_setup first)");
    if (kind) *kind = f.lvl ? f.lvl->order : 0;
    if (bandwidth) *bandwidth = f.lvl ? f.lvl->bandwidth : -1;
    if (nLevelSets) *nLevelSets = f.nPlanes;
    if (nEntries) *nEntries = f.lvl ? f.lvl->nEntries : (int64_t)f.nEnt * f.ncell;
    return 0;
}

int adflow_gpu_pc_download_ordering(int32_t* perm, long n)
{
    const PcFactor& f = pc_sel();
    if (!f.valid) return fail("pc_download_ordering: no factor (call adflow_gpu_pc_setup first)");
    if (!perm) return fail("pc_download_ordering: perm is NULL");
    if (n != f.ncell) return fail("pc_download_ordering: n = %ld, the factor has %ld cells", n, f.ncell);
    const bool ident = !f.lvl || f.lvl->order == 0;
    for (long a = 0; a < n; ++a) perm[a] = ident ? (int32_t)a : f.lvl->perm[(size_t)a];
    return 0;
}

int adflow_gpu_pc_set_mg(int levels, int nSmooth, int fillCoarse)
{
    if (levels < 1 || levels > 10)
        return fail("pc_set_mg: %d levels; the hierarchy takes 1 (no multigrid) to 10 levels (coarseRows(2:10) of amg.F90)", levels);
    if (nSmooth < 1) return fail("pc_set_mg: nSmooth = %d; the smoother takes at least one iteration", nSmooth);
    if (fillCoarse < 0 || fillCoarse > 2)
        return fail("pc_set_mg: fillCoarse = %d; the block ILU of the coarse levels takes 0, 1 or 2 levels of fill", fillCoarse);
    g_pc_mg[g_pc_slot].levels = levels;
    g_pc_mg[g_pc_slot].nSmooth = nSmooth;
    g_pc_mg[g_pc_slot].fillCoarse = fillCoarse;
    return 0;
}

int adflow_gpu_pc_set_its(int outer, int inner, int innerCoarse)
{
    if (outer < 1) return fail("pc_set_its: outer = %d; every count is at least 1 (1 = no iteration beyond the application)", outer);
    if (inner < 1) return fail("pc_set_its: inner = %d; every count is at least 1 (1 = no iteration beyond the application)", inner);
    if (innerCoarse < 1)
        return fail("pc_set_its: innerCoarse = %d; every count is at least 1 (1 = no iteration beyond the application)", innerCoarse);
    g_pc_its[g_pc_slot].outer = outer;
    g_pc_its[g_pc_slot].inner = inner;
    g_pc_its[g_pc_slot].innerCoarse = innerCoarse;
    return 0;
}

int adflow_gpu_pc_its_info(int32_t* outer, int32_t* inner, int32_t* innerCoarse, int64_t* matrixBytes)
{
    const PcFactor& f = pc_sel();
    if (!f.valid) return fail("pc_its_info: no factor (call adflow_gpu_pc_setup first)");
    if (outer) *outer = f.its.outer;
    if (inner) *inner = f.its.inner;
    if (innerCoarse) *innerCoarse = f.its.innerCoarse;
    if (matrixBytes) *matrixBytes = f.rich ? (int64_t)f.rich->matBytes : 0;
    return 0;
}

int adflow_gpu_pc_mg_info(int32_t* levels, int32_t* nSmooth, int32_t* fillCoarse, int64_t* cells)
{
    const PcFactor& f = pc_sel();
    if (!f.valid) return fail("pc_mg_info: no factor (call adflow_gpu_pc_setup first)");
    if (levels) *levels = f.mg ? (int32_t)f.mg->lv.size() : 1;
    if (nSmooth) *nSmooth = f.mg ? f.mg->nSmooth : 1;
    if (fillCoarse) *fillCoarse = f.mg ? f.mg->fillCoarse : 0;
    if (cells) {
        if (!f.mg) cells[0] = f.ncell;
        else
            for (size_t l = 0; l < f.mg->lv.size(); ++l) cells[l] = f.mg->lv[l].ncell;
    }
    return 0;
}

int adflow_gpu_pc_mg_download(int mgLevel, int nn, double* blocks)
{
    const PcFactor& f = pc_sel();
    if (!f.valid) return fail("pc_mg_download: no factor (call adflow_gpu_pc_setup first)");
    if (!f.mg) return fail("pc_mg_download: the factor of the selected slot has no hierarchy (adflow_gpu_pc_set_mg with levels > 1 first)");
    const PcMg& M = *f.mg;
    if (mgLevel < 1 || mgLevel > (int)M.lv.size())
        return fail("pc_mg_download: multigrid level %d; the hierarchy has the levels 1 .. %d", mgLevel, (int)M.lv.size());
    if (!blocks) return fail("pc_mg_download: blocks is NULL");
    const PcMgLevel& L = M.lv[mgLevel - 1];
    size_t s = 0;
    while (s < M.nnOf.size() && M.nnOf[s] != nn) ++s;
    if (s == M.nnOf.size()) return fail("pc_mg_download: block %d is not part of the hierarchy", nn);
    const JmBlk& q = L.hb[s];
    const size_t ncomp = (size_t)7 * f.nState * f.nState;
    std::vector<double> box(ncomp * q.nbox);
    HIPCHK(hipStreamSynchronize(g_stream));
    HIPCHK(hipMemcpy(box.data(), q.jac, box.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < ncomp; ++e)
        for (int k = 0; k < q.nz; ++k)
            for (int j = 0; j < q.ny; ++j)
                for (int i = 0; i < q.nx; ++i)
                    blocks[((e * q.nz + k) * q.ny + j) * q.nx + i] = box[e * q.nbox + (i + 2) + (long)(j + 2) * q.ldi + (long)(k + 2) * q.ldk];
    return 0;
}

int adflow_gpu_pc_release(int64_t* bytes)
{
    if (g_stream) HIPCHK(hipStreamSynchronize(g_stream));
    const int64_t n = pc_release(pc_sel());
    if (bytes) *bytes = n;
    return 0;
}

// z = M^-1 r or M^-T r with the selected factor, whatever its fill, for nv = 1 .. PC_MAXW columns ldr / ldz apart in the same launches
static int pc_factor_apply(const PcFactor& f, int transpose, const double* r, double* z, hipStream_t s, int nv = 1, long ldr = 0, long ldz = 0)
{
    if (f.lvl) {
        if (nv != 1) return fail("pc_apply: internal: the sweeps of the ILU over the level take one vector");
        return launch_pcl_apply(f.lvl->tab, f.nState, transpose, f.planeStart, r, z, s);
    }
    if (f.coupled) return launch_pcc_apply(f.tab, f.nState, transpose, f.planeStart, r, z, s, nv, ldr, ldz);
    if (f.fill > 0) return launch_pcf_apply(f.tab, f.nState, f.nEnt, transpose, f.planeStart, r, z, s, nv, ldr, ldz);
    return launch_pc_apply(f.tab, f.nState, transpose, f.planeStart, r, z, s, nv, ldr, ldz);
}

// The smoother of level l (0-based) of the hierarchy of f: Richardson from zero, nSmooth iterations, one ILU application each
// (setupShellPC):  x = M^-1 b,  then  x += M^-1 (b - A x).  t: a vector of the level that is free; the sweep turns it into the
// correction in place (the forward sweep has read all of its input before the backward sweep writes the first output).
// With inner iterations on the level (adflow_gpu_pc_set_its) every "one ILU application" is the Richardson L_l below, on w[] of the level.
static int pc_mg_smooth(const PcFactor& f, int l, int transpose, const double* b, double* x, double* t, hipStream_t s)
{
    const PcMg& M = *f.mg;
    const PcMgLevel& L = M.lv[l];
    const PcFactor& fac = l == 0 ? f : L.fac;
    const int nb = (int)L.hb.size();
    const int inner = l == 0 ? f.its.inner : f.its.innerCoarse;
    // inner > 1 (adflow_gpu_pc_set_its): the one ILU application becomes  y = L_l(c) = S(c; M_l, A_l, inner)  on the level's own matrix
    // (amgLocalPreConIts, amg.F90:534-615); w[0] carries its residual and, in place, its correction
    auto local = [&](const double* c, double* y) -> int {
        if (pc_factor_apply(fac, transpose, c, y, s)) return 1;
        for (int it = 1; it < inner; ++it) {
            launch_mg_residual(L.dtab, nullptr, nb, L.maxnx, L.maxny, L.maxnz, f.nState, transpose, M.sten, c, y, nullptr, L.w[0], s);
            if (pc_factor_apply(fac, transpose, L.w[0], L.w[0], s)) return 1;
            launch_gm_axpby(y, 1.0, L.w[0], 1.0, L.ncell * f.nState, s);
        }
        return 0;
    };
    if (local(b, x)) return 1;
    for (int it = 1; it < M.nSmooth; ++it) {
        launch_mg_residual(L.dtab, nullptr, nb, L.maxnx, L.maxny, L.maxnz, f.nState, transpose, M.sten, b, x, nullptr, t, s);
        if (inner == 1) {
            if (pc_factor_apply(fac, transpose, t, t, s)) return 1;
            launch_gm_axpby(x, 1.0, t, 1.0, L.ncell * f.nState, s);
        } else {
            if (local(t, L.w[1])) return 1;
            launch_gm_axpby(x, 1.0, L.w[1], 1.0, L.ncell * f.nState, s);
        }
    }
    return 0;
}

// y = MG(r, l) of amg.F90:712-759 for level l (0-based) of the hierarchy of f, which is not its last one: the coarse level first, the
// smoother of this level afterwards.  Launches on s only; the vectors are those of the levels (no allocation, no synchronise).
//   launches: restriction, the cycle or the smoother below, prolongation fused with the residual, the smoother, y += x
static int pc_mg_cycle(const PcFactor& f, int l, int transpose, const double* r, double* y, hipStream_t s)
{
    const PcMg& M = *f.mg;
    const PcMgLevel &F = M.lv[l], &C = M.lv[l + 1];
    const int nb = (int)F.hb.size(), nS = f.nState;
    launch_mg_restrict(F.dtab, C.dtab, nb, C.maxnx, C.maxny, C.maxnz, nS, r, C.v[0], s);
    if (l + 2 == (int)M.lv.size() ? pc_mg_smooth(f, l + 1, transpose, C.v[0], C.v[1], C.v[2], s)
                                  : pc_mg_cycle(f, l + 1, transpose, C.v[0], C.v[1], s))
        return 1;
    launch_mg_residual(F.dtab, C.dtab, nb, F.maxnx, F.maxny, F.maxnz, nS, transpose, M.sten, r, C.v[1], y, F.v[2], s);
    // r is dead from here: below level 1 it is v[0] of this level, which the smoother may use; level 1 has a v[0] of its own
    if (pc_mg_smooth(f, l, transpose, F.v[2], F.v[3], F.v[0], s)) return 1;
    launch_gm_axpby(y, 1.0, F.v[3], 1.0, F.ncell * nS, s);
    return 0;
}

// The one place an application of the selected slot is dispatched: the cycle of its hierarchy, or its factor
static int pc_apply_enqueue(int transpose, const double* r, double* z, hipStream_t s, int nv = 1, long ldr = 0, long ldz = 0)
{
    const PcFactor& f = pc_sel();
    if (f.mg && nv != 1) return fail("pc_apply: internal: the multigrid cycle takes one vector");
    if (!f.rich) return f.mg ? pc_mg_cycle(f, 0, transpose, r, z, s) : pc_factor_apply(f, transpose, r, z, s, nv, ldr, ldz);
    // The Richardson iterations of adflow_gpu_pc_set_its, from a zero guess, scale 1, no norm (transpose: A^T and M^-T throughout):
    //   local(b) = S(b; M, A_sub, inner):  y = M^-1 b,  then inner - 1 times  y += M^-1 (b - A_sub y)     (a hierarchy: its cycle)
    //   P(b):                              z = local(b),  then outer - 1 times  z += local(b - A_full z)
    // A_sub = A_full without the columns behind block faces for a factor with one subdomain per block.  The work vectors are those
    // of the setup (pc_ws_reserve for more than one column): launches on s only, no allocation, no synchronise.  No sweep runs in place.
    const PcRich& R = *f.rich;
    const long n = f.ncell * f.nState;
    if (nv > R.width) return fail("pc_apply: internal: the work vectors of the iterations serve %d columns, not %d", R.width, nv);
    auto work = [&](int q) { return R.work + (size_t)q * R.width * n; };
    auto add = [&](double* y, long ldy, const double* c) {
        for (int v = 0; v < nv; ++v) launch_gm_axpby(y + v * ldy, 1.0, c + v * n, 1.0, n, s);
    };
    const int wi = f.its.outer > 1 ? 2 : 0;       // the first work vector of the inner loop
    auto local = [&](const double* b, long ldb, double* y, long ldy) -> int {
        if (f.mg) return pc_mg_cycle(f, 0, transpose, b, y, s);
        if (pc_factor_apply(f, transpose, b, y, s, nv, ldb, ldy)) return 1;
        for (int it = 1; it < f.its.inner; ++it) {
            if (launch_rich_residual(R.tab, f.nState, transpose, !f.coupled, nv, b, ldb, y, ldy, work(wi), n, s)) return 1;
            if (pc_factor_apply(f, transpose, work(wi), work(wi + 1), s, nv, n, n)) return 1;
            add(y, ldy, work(wi + 1));
        }
        return 0;
    };
    if (local(r, ldr, z, ldz)) return 1;
    for (int it = 1; it < f.its.outer; ++it) {
        if (launch_rich_residual(R.tab, f.nState, transpose, 0, nv, r, ldr, z, ldz, work(0), n, s)) return 1;
        if (local(work(0), n, work(1), n)) return 1;
        add(z, ldz, work(1));
    }
    return 0;
}

// The work space of the selected factor for nv vectors at once: the part beyond the first vector is allocated at the first
// multi-vector application, kept at the widest group asked for, counted by adflow_gpu_pc_info and released with the factor
static int pc_ws_reserve(const char* who, int nv)
{
    PcFactor& f = pc_sel();
    if (nv <= f.wsWidth) return 0;
    HIPCHK(hipStreamSynchronize(g_stream));            // sweeps in the queue may still use the part that is replaced
    const size_t per = (size_t)f.ncell * f.nState * sizeof(double);
    if (f.tab.wsx) {
        (void)hipFree(f.tab.wsx);
        f.raw.erase(std::find(f.raw.begin(), f.raw.end(), (void*)f.tab.wsx));
        f.bytes -= per * (f.wsWidth - 1);
        f.tab.wsx = nullptr;
        f.wsWidth = 1;
    }
    void* p = nullptr;
    if (hipMalloc(&p, per * (nv - 1)) != hipSuccess) {
        (void)hipGetLastError();
        return fail("%s: cannot allocate %zu bytes of work space for %d vectors at once; the factor stands as it was", who, per * (nv - 1), nv);
    }
    f.raw.push_back(p);
    f.bytes += per * (nv - 1);
    f.tab.wsx = (double*)p;
    f.wsWidth = nv;
    // the work vectors of the Richardson iterations (adflow_gpu_pc_set_its) at the same width
    if (f.rich && f.rich->nWork > 0) {
        PcRich& R = *f.rich;
        void* q = nullptr;
        if (hipMalloc(&q, per * R.nWork * nv) != hipSuccess) {
            (void)hipGetLastError();
            return fail("%s: cannot allocate %zu bytes of work space for the iterations of %d vectors at once; the factor stands and "
                        "applies one vector at a time", who, per * R.nWork * nv, nv);
        }
        (void)hipFree(R.work);
        *std::find(f.raw.begin(), f.raw.end(), (void*)R.work) = q;
        f.bytes += per * R.nWork * (nv - R.width);
        R.work = (double*)q;
        R.width = nv;
    }
    return 0;
}

// the columns in groups of at most PC_MAXW, each group one chain of launches; one column is the application it always was
static int pc_apply_multi_enqueue(const char* who, int transpose, int nvec, const double* r, long ldr, double* z, long ldz, hipStream_t s)
{
    // fill 2: one column per chain of launches, the kernels of the single entry -- its sweeps of several vectors are not shipped
    // (kernels_pc_fill.hip), so there the multi entry costs what the single calls cost
    // a hierarchy: one column per cycle as well (a cycle of several vectors is not built)
    // the ILU over the level: one column per chain as well, as at fill 2
    const int width = (pc_sel().fill == 2 || pc_sel().mg || pc_sel().lvl) ? 1 : (int)PC_MAXW;
    if (pc_ws_reserve(who, std::min(width, nvec))) return 1;
    for (int c = 0; c < nvec; c += width)
        if (pc_apply_enqueue(transpose, r + c * ldr, z + c * ldz, s, std::min(width, nvec - c), ldr, ldz)) return 1;
    return 0;
}

static int pc_check(const char* who, int level, const double* r, const double* z, long n, bool rows = true)
{
    if (need_ready()) return 1;
    if (!pc_sel().valid) return fail("%s: no factor (call adflow_gpu_pc_setup first)", who);
    if (level != pc_sel().level) return fail("%s: level %d is not the level of the factor (%d)", who, level, pc_sel().level);
    if (!r || !z) return fail("%s: %s is NULL", who, !r ? "the right-hand side" : "the result");
    if (r == z) return fail("%s: right-hand side and result are the same vector (not done in place)", who);
    if (rows && n != pc_sel().ncell * pc_sel().nState)
        return fail("%s: n=%ld but the factor of level %d has %ld rows (nState = %d x %ld owned cells)", who, n, level,
                    pc_sel().ncell * pc_sel().nState, pc_sel().nState, pc_sel().ncell);
    return 0;
}

int adflow_gpu_pc_apply_dev(int level, int transpose, const double* d_r, double* d_z, long n)
{
    if (pc_check("pc_apply", level, d_r, d_z, n)) return 1;
    if (pc_apply_enqueue(transpose, d_r, d_z, g_stream)) return 1;
    return sync_and_check();
}

int adflow_gpu_pc_apply(int level, int transpose, const double* r, double* z, long n)
{
    Stage s;
    return pc_check("pc_apply", level, r, z, n) || stage_open(&s, n, 2) || s.in(0, r) || pc_apply_enqueue(transpose, s[0], s[1], g_stream) ||
           s.out(z, 1) || s.done();
}

int adflow_gpu_pc_apply_multi_dev(int level, int transpose, int nvec, const double* d_R, long ldr, double* d_Z, long ldz, long n)
{
    if (multi_check("pc_apply_multi", nvec, d_R, ldr, d_Z, ldz, n) || pc_check("pc_apply_multi", level, d_R, d_Z, n)) return 1;
    if (pc_apply_multi_enqueue("pc_apply_multi", transpose, nvec, d_R, ldr, d_Z, ldz, g_stream)) return 1;
    return sync_and_check();
}

int adflow_gpu_pc_apply_multi(int level, int transpose, int nvec, const double* R, long ldr, double* Z, long ldz, long n)
{
    Stage s;
    return multi_check("pc_apply_multi", nvec, R, ldr, Z, ldz, n) || pc_check("pc_apply_multi", level, R, Z, n) ||
           stage_open(&s, n, 2 * nvec) || stage_in_columns(s, 0, R, ldr, nvec) ||
           pc_apply_multi_enqueue("pc_apply_multi", transpose, nvec, s[0], n, s[nvec], n, g_stream) ||
           stage_out_columns(s, Z, ldz, nvec, nvec) || s.done();
}

// GMRES(restart) on  A M^-1 u = b, x = M^-1 u  (transpose: A^T M^-T), A = adflow_gpu_jacobian_mult with the matrix on the device,
// M = the factor.  Basis, dots and updates on the device (one launch per basis vector of a modified Gram-Schmidt step, one
// download of the new Hessenberg column per step); Hessenberg matrix and Givens rotations on the host.
// op(v, y) enqueues y = A v: jm_mult_enqueue on the assembled matrix, or the matrix-free operator of ANK (ank_mult_enqueue).
// The least-squares problem of one right-hand side on the host: the Hessenberg matrix column by column through its Givens rotations
struct GmLsq {
    std::vector<std::vector<double>> R;
    std::vector<double> cs, sn, g, y;
    explicit GmLsq(int m) : R(m), cs(m), sn(m), g(m + 1), y(m) {}
    void start(double beta)
    {
        g.assign(g.size(), 0.0);
        g[0] = beta;
    }
    // column j: H[i stride], i = 0 .. j, and the norm hn of the new vector; returns the residual norm of the recurrence
    double column(const double* H, long stride, int j, double hn)
    {
        std::vector<double>& c = R[j];
        c.resize(j + 1);
        for (int i = 0; i <= j; ++i) c[i] = H[i * stride];
        for (int i = 0; i < j; ++i) {
            const double a = c[i], b = c[i + 1];
            c[i] = cs[i] * a + sn[i] * b;
            c[i + 1] = -sn[i] * a + cs[i] * b;
        }
        const double d = hypot(c[j], hn);
        cs[j] = d > 0.0 ? c[j] / d : 1.0;
        sn[j] = d > 0.0 ? hn / d : 0.0;
        c[j] = d;
        g[j + 1] = -sn[j] * g[j];
        g[j] = cs[j] * g[j];
        return fabs(g[j + 1]);
    }
    // y: the coefficients of the first k basis vectors
    void solve(int k)
    {
        for (int i = k - 1; i >= 0; --i) {
            double t = g[i];
            for (int q = i + 1; q < k; ++q) t -= R[q][i] * y[q];
            y[i] = R[i][i] != 0.0 ? t / R[i][i] : 0.0;
        }
    }
};

typedef std::function<int(const double*, double*)> GmOperator;
static int gm_solve(const char* who, const GmOperator& op, int transpose, const double* d_b, double* d_x, long n, int restart, int maxIts,
                    double rtol, double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    const int m = std::max(1, std::min(restart, std::max(maxIts, 1)));
    DevBuf buf;
    // m + 1 basis vectors, zt, tv; then two buffers of partial sums (read one, write the other) and the Hessenberg column
    const size_t nv = (size_t)(m + 3) * n, nred = 2 * GM_PARTS + (size_t)m + 2;
    HIPCHK(hipMalloc(&buf.p, (nv + nred) * sizeof(double)));
    double* V = (double*)buf.p;
    double *zt = V + (size_t)(m + 1) * n, *tv = zt + n, *red = tv + n, *P[2] = {red, red + GM_PARTS}, *dH = red + 2 * GM_PARTS;
    std::vector<double> H(m + 2);
    hipStream_t s = g_stream;
    auto norm = [&](const double* a, double* out) -> int {
        launch_gm_mgs(const_cast<double*>(a), nullptr, nullptr, nullptr, P[0], nullptr, n, s);
        launch_gm_sum(P[0], n, dH, s);
        HIPCHK(hipMemcpyAsync(H.data(), dH, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        *out = sqrt(std::max(H[0], 0.0));
        if (!(H[0] == H[0])) *out = H[0];            // NaN stays NaN
        return 0;
    };
    auto residual = [&](double* r, bool zeroX) -> int {          // r = b - A x
        if (zeroX) {
            HIPCHK(hipMemcpyAsync(r, d_b, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
            return 0;
        }
        if (op(d_x, r)) return 1;
        launch_gm_axpby(r, 1.0, d_b, -1.0, n, s);
        return 0;
    };
    double bnorm = 0.0, beta = 0.0, res = 0.0;
    if (norm(d_b, &bnorm)) return 1;
    if (!(bnorm == bnorm)) return fail("%s: the right-hand side is not finite", who);
    const double tol = std::max(rtol * bnorm, atol);
    if (!useGuess) HIPCHK(hipMemsetAsync(d_x, 0, sizeof(double) * n, s));
    int total = 0;
    bool first = true, zeroX = !useGuess;
    GmLsq q(m);
    for (;;) {
        if (residual(V, zeroX)) return 1;
        if (norm(V, &beta)) return 1;
        if (!(beta == beta)) return fail("%s: the residual is not finite after %d iterations", who, total);
        if (first) { if (rnorm0) *rnorm0 = beta; first = false; }
        res = beta;
        if (beta <= tol || total >= maxIts) break;
        launch_gm_axpby(V, 1.0 / beta, V, 0.0, n, s);
        q.start(beta);
        int k = 0;
        bool stop = false;
        for (int j = 0; j < m && !stop; ++j) {
            double* w = V + (size_t)(j + 1) * n;
            if (pc_apply_enqueue(transpose, V + (size_t)j * n, zt, s)) return 1;
            if (op(zt, w)) return 1;
            launch_gm_mgs(w, nullptr, nullptr, V, P[0], nullptr, n, s);
            for (int i = 1; i <= j; ++i)
                launch_gm_mgs(w, V + (size_t)(i - 1) * n, P[(i - 1) & 1], V + (size_t)i * n, P[i & 1], dH + (i - 1), n, s);
            launch_gm_mgs(w, V + (size_t)j * n, P[j & 1], nullptr, P[(j + 1) & 1], dH + j, n, s);
            launch_gm_sum(P[(j + 1) & 1], n, dH + j + 1, s);
            HIPCHK(hipMemcpyAsync(H.data(), dH, sizeof(double) * (j + 2), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            const double hn = sqrt(std::max(H[j + 1], 0.0));
            if (!(H[j + 1] == H[j + 1])) return fail("%s: the Krylov vector of iteration %d is not finite", who, total + 1);
            res = q.column(H.data(), 1, j, hn);
            ++total;
            k = j + 1;
            if (hn > 0.0) launch_gm_axpby(w, 1.0 / hn, w, 0.0, n, s);
            stop = res <= tol || total >= maxIts || !(hn > 0.0);
        }
        q.solve(k);
        for (int i = 0; i < k; ++i) launch_gm_axpby(tv, q.y[i], V + (size_t)i * n, i == 0 ? 0.0 : 1.0, n, s);
        if (k > 0) {
            if (pc_apply_enqueue(transpose, tv, zt, s)) return 1;
            launch_gm_axpby(d_x, 1.0, zt, 1.0, n, s);
            zeroX = false;
        }
        if (stop) {
            // converged on the recurrence (or out of iterations): the reported norm is the true residual
            if (residual(V, false)) return 1;
            if (norm(V, &res)) return 1;
            break;
        }
    }
    if (its) *its = total;
    if (rnorm) *rnorm = res;
    HIPCHK(hipGetLastError());
    return 0;
}

// The refusals every solve shares: those of the library and the communicator first, those of the caps last, the solve's own about its
// operands between them.  `who` is the entry, multDev the product a host's KSP would call
static int gm_check_ranks(const char* who, const char* multDev)
{
    if (need_ready()) return 1;
#ifndef ADFLOW_NO_RCCL
    if (g_nranks > 1)
        return fail("%s: %d ranks in the communicator; the dot products of the solver are not reduced across ranks (use the "
                    "host's KSP with %s and adflow_gpu_pc_apply_dev)", who, g_nranks, multDev);
#else
    (void)multDev;
#endif
    return 0;
}

static int gm_check_caps(const char* who, int restart, int maxIts, double rtol, double atol)
{
    if (restart < 1 || maxIts < 0) return fail("%s: restart = %d, maxIts = %d", who, restart, maxIts);
    if (!(rtol >= 0.0) || !(atol >= 0.0)) return fail("%s: rtol = %g, atol = %g", who, rtol, atol);
    return 0;
}

static int gm_check(int level, const double* b, const double* x, long n, int restart, int maxIts, double rtol, double atol)
{
    if (gm_check_ranks("gmres_solve", "adflow_gpu_jacobian_mult_dev")) return 1;
    if (!g_jac_valid) return fail("gmres_solve: no assembled Jacobian (call adflow_gpu_fd_jacobian first)");
    if (pc_check("gmres_solve", level, b, x, n, false)) return 1;
    if (g_jac.nState != pc_sel().nState)
        return fail("gmres_solve: the factor was set up for nState = %d, the assembled matrix has nState = %d", pc_sel().nState, g_jac.nState);
    if (jm_check(level, b, x, n)) return 1;
    if (n != pc_sel().ncell * pc_sel().nState) return fail("gmres_solve: n=%ld but the factor has %ld rows", n, pc_sel().ncell * pc_sel().nState);
    return gm_check_caps("gmres_solve", restart, maxIts, rtol, atol);
}

int adflow_gpu_gmres_solve_dev(int level, int transpose, const double* d_b, double* d_x, long n, int restart, int maxIts, double rtol,
                               double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    if (gm_check(level, d_b, d_x, n, restart, maxIts, rtol, atol)) return 1;
    const GmOperator op = [=](const double* v, double* y) { return jm_mult_enqueue(level, transpose, v, y); };
    return gm_solve("gmres_solve", op, transpose, d_b, d_x, n, restart, maxIts, rtol, atol, useGuess, its, rnorm0, rnorm);
}

int adflow_gpu_gmres_solve(int level, int transpose, const double* b, double* x, long n, int restart, int maxIts, double rtol,
                           double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    if (gm_check(level, b, x, n, restart, maxIts, rtol, atol)) return 1;
    DevBuf buf;                        // b and x of this call, not g_vec_dev
    HIPCHK(hipMalloc(&buf.p, sizeof(double) * 2 * n));
    const Stage s{n, (double*)buf.p};
    if (s.in(0, b) || (useGuess && s.in(1, x))) return 1;
    const GmOperator op = [=](const double* v, double* y) { return jm_mult_enqueue(level, transpose, v, y); };
    return gm_solve("gmres_solve", op, transpose, s[0], s[1], n, restart, maxIts, rtol, atol, useGuess, its, rnorm0, rnorm) ||
           s.out(x, 1) || s.done();
}

// ---- matrix-free exact products by forward mode: y = (dR/dw) x without an assembled matrix ------------------------------------------
// The shell matrix the reference solves the direct equations on (useMatrixFreedRdw, pyADflow.py:5918; createPETScVars makes dRdwT a
// shell, adjointAPI.F90:1199-1214): its forward product dRdwMatMult (:1050-1128) is ONE master_d with the vector as seed.  Here: the
// vector goes through the halo'd scratch array and the 2-layer exchange of jacobian_mult (the column rule is the same), the seed
// kernel writes the dual state from it, block_res_state_d runs once, and the read-out kernel takes the derivative part of the scaled
// residual into y.  The evaluation is the one a coloured pass of adflow_gpu_fd_jacobian(flags | USE_AD) runs, so y is the product
// with the matrix that call would assemble.
namespace {
struct JfSetup {
    JacSpec J;
    unsigned resFlags = 0;
    bool pc = false, viscPC = false, turbBC = false, rans = false;
};
}  // namespace

// the refusals of a product; on success S says what the flags select
static int jf_check(const char* who, int level, unsigned flags, const double* x, const double* y, long n, JfSetup* S)
{
    if (need_ready()) return 1;
    if (jac_check_args(level, flags | ADFLOW_JAC_USE_AD, 0.0, who, "")) return 1;
    if (!x || !y) return fail("%s: %s is NULL", who, !x ? "x" : "y");
    if (x == y) return fail("%s: x and y are the same vector (the product is not done in place)", who);
    S->rans = g_opts.equations == ADFLOW_RANS;
    jac_spec(flags & ~(ADFLOW_JAC_USE_AD | ADFLOW_JAC_APPROX_SA), S->rans || g_opts.equations == ADFLOW_NS, S->rans, &S->J);
    long cells = 0;
    int rc = for_level(level, [&](Block* b) {
        cells += (long)b->v.nx * b->v.ny * b->v.nz;
        return 0;
    });
    if (rc) return rc;
    if (n != cells * S->J.nState)
        return fail("%s: n=%ld but the operator of level %d has %ld rows (nState = %d x %ld owned cells)", who, n, level,
                    cells * S->J.nState, S->J.nState, cells);
    CommPattern* cp;
    if (jm_pattern_of(level, S->J.lStart, S->J.nState, who, &cp)) return 1;
    // the switches of adflow_gpu_fd_jacobian
    S->pc = (flags & ADFLOW_JAC_PC) != 0;
    S->viscPC = (flags & ADFLOW_JAC_VISC_PC) != 0;
    S->turbBC = S->rans && !(flags & ADFLOW_JAC_FROZEN_TURB);
    S->resFlags = 0;
    if (!(flags & ADFLOW_JAC_TURB_ONLY)) S->resFlags |= ADFLOW_RES_FLOW;
    if (S->turbBC) S->resFlags |= ADFLOW_RES_TURB;
    if (S->turbBC && (flags & ADFLOW_JAC_APPROX_SA)) S->resFlags |= ADFLOW_RES_APPROX_SA;
    if (S->pc) S->resFlags |= ADFLOW_RES_DISS_APPROX | ADFLOW_RES_VISC_APPROX;
    return 0;
}

// what one linearisation point needs (PcSwitchGuard in force): whalo2 of the state, the frozen shock sensor of the preconditioner
// matrix, the passive dual arrays, the scratch of the vector.  The host waits only where the slab or the scratch is laid out, or sync
static int jf_prepare(const char* who, int level, const JfSetup& S, bool sync)
{
    if (g_comm.count(std::make_pair(level, 2)))
        if (halo_exchange_enqueue(level, 1, S.rans ? 6 : 5, 1, 1, 2)) return 1;
    if (S.pc && reference_shock_sensor_enqueue(level)) return 1;
    if (ad_prepare(level, sync)) return 1;
    return jm_layout(g_jf, level, S.J.nState, 1, false, who);
}

// seed, evaluate, read out (PcSwitchGuard in force, jf_prepare done)
static int jf_product_enqueue(const char* who, int level, const JfSetup& S, const double* d_x, double* d_y)
{
    CommPattern* cp;
    if (jm_pattern_of(level, S.J.lStart, S.J.nState, who, &cp)) return 1;
    if (jm_scatter_x(g_jf, d_x, 1, 0) || jm_exchange_x(g_jf, cp, 1)) return 1;
    const KParams kp = res_kparams(level, S.resFlags);
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level)
            ad_launch_seed_vector(kv.second->v, g_ad[kv.second].v, g_jf.h[std::get<2>(kv.first)].xs, S.J.lStart, S.J.nState, kp, g_stream);
    if (block_res_state_enqueue(DUAL, level, S.resFlags, S.turbBC, S.viscPC, true)) return 1;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level)
            ad_launch_jf_readout(g_ad[kv.second].v, d_y, g_jf.h[std::get<2>(kv.first)].vecOff, S.J.lStart, S.J.nState, g_opts.turbResScale,
                                 g_stream);
    return 0;
}

// after the last product of a call: a failed call, or tuning "ad_cache" = 0, gives the slab back (the queue is drained first)
static int jf_finish(int rc)
{
    if (rc || !g_ad_cache) {
        (void)hipStreamSynchronize(g_stream);
        ad_drop();
    }
    return rc;
}

static int jf_mult_enqueue(const char* who, int level, const JfSetup& S, const double* d_x, double* d_y, bool sync)
{
    PcSwitchGuard switches(S.pc);
    int rc = jf_prepare(who, level, S, sync);
    if (!rc) rc = jf_product_enqueue(who, level, S, d_x, d_y);
    return jf_finish(rc);
}

int adflow_gpu_jacfree_mult_dev(int level, unsigned flags, const double* d_x, double* d_y, long n)
{
    JfSetup S;
    if (jf_check("jacfree_mult", level, flags, d_x, d_y, n, &S)) return 1;
    if (jf_mult_enqueue("jacfree_mult", level, S, d_x, d_y, !g_async)) return 1;
    return sync_and_check();
}

int adflow_gpu_jacfree_mult(int level, unsigned flags, const double* x, double* y, long n)
{
    JfSetup S;
    Stage s;
    return jf_check("jacfree_mult", level, flags, x, y, n, &S) || stage_open(&s, n, 2) || s.in(0, x) ||
           jf_mult_enqueue("jacfree_mult", level, S, s[0], s[1], false) || s.out(y, 1) || s.done();
}

// GMRES on the shell matrix: the KSP of solveDirectForRHS (adjointAPI.F90) with dRdwMatMult as operator and the factor of the selected
// slot as right preconditioner, never transposed.  One preparation, then every product only seeds, evaluates and reads out
static int jf_solve_check(int level, unsigned flags, const double* b, const double* x, long n, int restart, int maxIts, double rtol,
                          double atol, JfSetup* S)
{
    if (gm_check_ranks("jacfree_solve", "adflow_gpu_jacfree_mult_dev")) return 1;
    if (pc_check("jacfree_solve", level, b, x, n, false)) return 1;
    if (jf_check("jacfree_solve", level, flags, b, x, n, S)) return 1;
    if (S->J.nState != pc_sel().nState)
        return fail("jacfree_solve: the factor was set up for nState = %d, the flags select nState = %d", pc_sel().nState, S->J.nState);
    if (n != pc_sel().ncell * pc_sel().nState) return fail("jacfree_solve: n=%ld but the factor has %ld rows", n, pc_sel().ncell * pc_sel().nState);
    return gm_check_caps("jacfree_solve", restart, maxIts, rtol, atol);
}

static int jf_solve_run(int level, const JfSetup& S, const double* d_b, double* d_x, long n, int restart, int maxIts, double rtol,
                        double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    PcSwitchGuard switches(S.pc);
    int rc = jf_prepare("jacfree_solve", level, S, true);
    const GmOperator op = [&](const double* v, double* y) { return jf_product_enqueue("jacfree_solve", level, S, v, y); };
    if (!rc) rc = gm_solve("jacfree_solve", op, 0, d_b, d_x, n, restart, maxIts, rtol, atol, useGuess, its, rnorm0, rnorm);
    return jf_finish(rc);
}

int adflow_gpu_jacfree_solve_dev(int level, unsigned flags, const double* d_b, double* d_x, long n, int restart, int maxIts, double rtol,
                                 double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    JfSetup S;
    if (jf_solve_check(level, flags, d_b, d_x, n, restart, maxIts, rtol, atol, &S)) return 1;
    if (jf_solve_run(level, S, d_b, d_x, n, restart, maxIts, rtol, atol, useGuess, its, rnorm0, rnorm)) return 1;
    return sync_and_check();
}

int adflow_gpu_jacfree_solve(int level, unsigned flags, const double* b, double* x, long n, int restart, int maxIts, double rtol,
                             double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    JfSetup S;
    if (jf_solve_check(level, flags, b, x, n, restart, maxIts, rtol, atol, &S)) return 1;
    DevBuf buf;                        // b and x of this call, not g_vec_dev
    HIPCHK(hipMalloc(&buf.p, sizeof(double) * 2 * n));
    const Stage s{n, (double*)buf.p};
    if (s.in(0, b) || (useGuess && s.in(1, x))) return 1;
    return jf_solve_run(level, S, s[0], s[1], n, restart, maxIts, rtol, atol, useGuess, its, rnorm0, rnorm) || s.out(x, 1) || s.done();
}

// ---- derivatives of the surface integration with respect to the state (kernels_wallint.hip in namespace adj) ----------------------
// wallIntegrationFace_d behind the front of block_res_state_d: what master_d adds to funcsDot for the wall subfaces, and -- as a
// coloured sweep of the same pass -- what master_b adds to wbar.  The functions depend on the state through the closures, the boundary
// conditions, the nodal gradients of the wall node planes and the stress of the wall faces: the pass runs those on the dual arrays and
// nothing else (no time step, no flux kernel).  The flags select the state range as for the matrix-free products.
static int wd_check_flags(const char* who, unsigned flags)
{
    if (flags & (ADFLOW_JAC_PC | ADFLOW_JAC_VISC_PC | ADFLOW_JAC_APPROX_SA))
        return fail("%s: ADFLOW_JAC_PC, ADFLOW_JAC_VISC_PC and ADFLOW_JAC_APPROX_SA select approximations of the fluxes, which the "
                    "derivatives of the surface integration do not run (flags 0x%x)", who, flags);
    return 0;
}

// turbulence and mean-flow boundary conditions and the nodal gradients of the wall node planes, on the dual arrays the seed launch
// filled (state and closures).  The dual face kernels take the stress from there
static int wd_front_enqueue(int level, const JfSetup& S, const KParams& kp, bool flow)
{
    // (the terms of a flow subface read rho, the velocities, p and gamma of the halo and of the first cell: the flow boundary
    //  conditions, and neither the turbulence ones nor a nodal gradient)
    if (flow) return DUAL.bcs(level, kp, false);
    if (DUAL.bcs(level, kp, S.turbBC)) return 1;
    BcPlan* pl;
    if (bc_plan(level, &pl)) return 1;
    if (g_opts.equations != ADFLOW_EULER) ad_launch_wall_node_grad(g_ad_tab, pl->d_ent, pl->d_order, pl->wall, g_stream);
    return 0;
}

// the dual arrays and the scratch of the vector.  Unlike jf_prepare no whalo2 of the state: like the integration itself the pass reads
// the halos of the state as they are on the device (whalo2 would also re-form the energy of the owned cells), and writes none of them
static int wd_prepare(const char* who, int level, const JfSetup& S, bool sync)
{
    if (ad_prepare(level, sync)) return 1;
    return jm_layout(g_jf, level, S.J.nState, 1, false, who);
}

// F: the parameters of the flow subfaces where L is their record, NULL for the walls (then P holds)
static int wd_fwd_enqueue(const char* who, int level, const JfSetup& S, const WiPar& P, const FiPar* F, WiLevel& L, int nG, const double* d_x,
                          double* d_out, double* d_outDot, bool sync)
{
    const int nface = (int)L.faces.size();
    if (F && d_out) {
        // the value parts of the flow entry are the integration itself, by the plain kernels in the same queue: the dual pass forms
        // the pressure of every cell again from its energy and would differ from adflow_gpu_flow_integrate in the last bits
        LevelTab t;
        if (level_tab(level, &t)) return 1;
        launch_flowint(t.tab, L.d_faces, nface, L.maxOwned, *F, L.part, L.d_member, nG, d_out, g_stream);
        d_out = nullptr;
    }
    if (nface == 0) {                  // no subface: the neutral elements and a zero derivative
        if (F) ad_launch_flowint_fwd(nullptr, nullptr, 0, 0, *F, nullptr, L.d_member, nG, d_out, d_outDot, g_stream);
        else ad_launch_wallint_fwd(nullptr, nullptr, 0, 0, P, KParams(), nullptr, L.d_member, nG, d_out, d_outDot, g_stream);
        return 0;
    }
    if (!L.partD) {
        const size_t nwg = (size_t)wallint_groups_per_face(L.maxOwned) * nface;
        if (wi_alloc(L, &L.partD, 2 * sizeof(double) * L.nq * nwg)) return 1;
    }
    int rc = wd_prepare(who, level, S, sync);
    const KParams kp = res_kparams(level, S.resFlags);
    CommPattern* cp = nullptr;
    if (!rc) rc = jm_pattern_of(level, S.J.lStart, S.J.nState, who, &cp);
    if (!rc) rc = jm_scatter_x(g_jf, d_x, 1, 0) || jm_exchange_x(g_jf, cp, 1);
    if (!rc) {
        for (auto& kv : g_blocks)
            if (std::get<0>(kv.first) == level)
                ad_launch_seed_vector(kv.second->v, g_ad[kv.second].v, g_jf.h[std::get<2>(kv.first)].xs, S.J.lStart, S.J.nState, kp, g_stream);
        rc = wd_front_enqueue(level, S, kp, F != nullptr);
    }
    if (!rc) {
        if (F) ad_launch_flowint_fwd(g_ad_tab, L.d_faces, nface, L.maxOwned, *F, L.partD, L.d_member, nG, d_out, d_outDot, g_stream);
        else ad_launch_wallint_fwd(g_ad_tab, L.d_faces, nface, L.maxOwned, P, kp, L.partD, L.d_member, nG, d_out, d_outDot, g_stream);
    }
    return jf_finish(rc);
}

static int wd_fwd(const char* who, int level, unsigned flags, const double* x, long n, const double* par, int nGroups, const int32_t* famLists,
                  int ldFam, double* out, double* outDot, bool dev, bool flow = false)
{
    if (need_ready()) return 1;
    if (!x || !outDot) return fail("%s: %s is NULL", who, !x ? "x" : "outDot");
    if (wd_check_flags(who, flags)) return 1;
    JfSetup S;
    if (jf_check(who, level, flags, x, outDot, n, &S)) return 1;
    WiPar P;
    FiPar FP;
    const FiPar* F = flow ? &FP : nullptr;
    WiLevel* L;
    int nG;
    if (flow ? fi_setup(who, level, par, nGroups, famLists, ldFam, &FP, &L, &nG)
             : wi_setup(who, level, par, nGroups, famLists, ldFam, false, &P, &L, &nG))
        return 1;
    const size_t no = (size_t)ADFLOW_WALLINT_STRIDE * nG;
    if (dev) {
        if (wd_fwd_enqueue(who, level, S, P, F, *L, nG, x, out, outDot, !g_async)) return 1;
        return sync_and_check();
    }
    if (nG > L->dotGroups) {
        HIPCHK(hipStreamSynchronize(g_stream));
        if (L->d_dot) {                 // the smaller buffer goes: the record holds one
            L->allocs.erase(std::find(L->allocs.begin(), L->allocs.end(), (void*)L->d_dot));
            (void)hipFree(L->d_dot);
            L->bytes -= (int64_t)(2 * sizeof(double) * ADFLOW_WALLINT_STRIDE) * L->dotGroups;
            L->d_dot = nullptr; L->dotGroups = 0;
        }
        void* raw = nullptr;
        if (wi_alloc(*L, &raw, 2 * sizeof(double) * no)) return 1;
        L->d_dot = (double*)raw;
        L->dotGroups = nG;
    }
    Stage s;
    if (stage_open(&s, n, 1) || s.in(0, x)) return 1;
    // (the flow entry forms its value parts with two launches of their own: only where the caller asks for them)
    if (wd_fwd_enqueue(who, level, S, P, F, *L, nG, s[0], (flow && !out) ? nullptr : L->d_dot, L->d_dot + no, false)) return 1;
    if (out && s.scalars(out, L->d_dot, (long)no)) return 1;
    return s.scalars(outDot, L->d_dot + no, (long)no) || s.done();
}

int adflow_gpu_wall_integrate_fwd(int level, unsigned flags, const double* x, long n, const double* par, int nGroups, const int32_t* famLists,
                                  int ldFam, double* out, double* outDot)
{
    return wd_fwd("wall_integrate_fwd", level, flags, x, n, par, nGroups, famLists, ldFam, out, outDot, false);
}

int adflow_gpu_wall_integrate_fwd_dev(int level, unsigned flags, const double* d_x, long n, const double* par, int nGroups,
                                      const int32_t* famLists, int ldFam, double* d_out, double* d_outDot)
{
    return wd_fwd("wall_integrate_fwd_dev", level, flags, d_x, n, par, nGroups, famLists, ldFam, d_out, d_outDot, true);
}

// the buffers of the transposed product for nS state variables and nv weight sets: the halo'd result ys of every block (nS x nv
// components), the level's table per set, the weights and the contracted derivatives of the faces
static int wd_bar_layout(const char* who, int level, WiLevel& L, int nS, int nv)
{
    if (L.barTab && L.barNS == nS && L.barNv == nv) return 0;
    HIPCHK(hipStreamSynchronize(g_stream));
    for (void* p : L.barAllocs) (void)hipFree(p);
    L.bytes -= L.barBytes;
    L.barBytes = 0;
    L.barAllocs.clear(); L.barYs.clear(); L.barYsBytes.clear();
    L.barTab = nullptr; L.d_wq = L.d_g = nullptr; L.wq.clear(); L.barNS = L.barNv = 0;
    auto alloc = [&](void** p, size_t bytes) {
        if (hipMalloc(p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail("%s: cannot allocate %zu bytes for the transposed product of %d weight sets", who, bytes, nv);
        }
        L.barAllocs.push_back(*p);
        L.barBytes += (int64_t)bytes;
        L.bytes += (int64_t)bytes;
        return 0;
    };
    int maxnn = 0;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == level) maxnn = std::max(maxnn, std::get<2>(kv.first));
    const size_t nt = (size_t)maxnn + 1;
    std::vector<JmBlk> h(nt);
    memset(h.data(), 0, sizeof(JmBlk) * nt);
    L.barYs.assign(nt, nullptr);
    L.barYsBytes.assign(nt, 0);
    L.barNx = L.barNy = L.barNz = 0;
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level) continue;
        const BlkView& v = kv.second->v;
        void* raw = nullptr;
        if (alloc(&raw, (size_t)v.nbox * nS * nv * sizeof(double) + 256)) return 1;
        JmBlk& q = h[std::get<2>(kv.first)];
        q.nx = v.nx; q.ny = v.ny; q.nz = v.nz; q.il = v.il; q.jl = v.jl; q.kl = v.kl; q.ib = v.ib; q.jb = v.jb; q.kb = v.kb;
        q.ldi = v.ldi; q.ldk = v.ldk; q.nbox = v.nbox;
        q.ys = (double*)raw + ADF_PAD0;
        L.barYs[std::get<2>(kv.first)] = (double*)raw;
        L.barYsBytes[std::get<2>(kv.first)] = (size_t)v.nbox * nS * nv * sizeof(double) + 256;
        L.barNx = std::max(L.barNx, v.nx); L.barNy = std::max(L.barNy, v.ny); L.barNz = std::max(L.barNz, v.nz);
    }
    long off = 0;
    for (auto& q : h) { q.vecOff = off; off += (long)q.nx * q.ny * q.nz * nS; }
    std::vector<JmBlk> ht(nt * nv);
    for (int c = 0; c < nv; ++c)
        for (size_t q = 0; q < nt; ++q) {
            ht[c * nt + q] = h[q];
            if (h[q].ys) ht[c * nt + q].ys += (size_t)h[q].nbox * nS * c;
        }
    void* raw = nullptr;
    if (alloc(&raw, sizeof(JmBlk) * ht.size())) return 1;
    L.barTab = (JmBlk*)raw;
    HIPCHK(hipMemcpy(L.barTab, ht.data(), sizeof(JmBlk) * ht.size(), hipMemcpyHostToDevice));
    if (alloc(&raw, sizeof(double) * std::max<size_t>(1, (size_t)nv * L.faces.size() * L.nq))) return 1;
    L.d_wq = (double*)raw;
    if (alloc(&raw, sizeof(double) * std::max<size_t>(1, (size_t)nv * L.nOwned))) return 1;
    L.d_g = (double*)raw;
    L.barSlots = maxnn; L.barNS = nS; L.barNv = nv;
    return 0;
}

static int wd_bwd_enqueue(const char* who, int level, const JfSetup& S, const WiPar& P, const FiPar* F, WiLevel& L,
                          const std::vector<double>& wq, int nRhs, double* d_wbar, long n, long ld, bool sync)
{
    const int nface = (int)L.faces.size();
    if (nface == 0) {
        for (int r = 0; r < nRhs; ++r) HIPCHK(hipMemsetAsync(d_wbar + r * ld, 0, sizeof(double) * n, g_stream));
        return 0;
    }
    const int nS = S.J.nState;
    if (wd_bar_layout(who, level, L, nS, nRhs)) return 1;
    if (wq != L.wq) {
        HIPCHK(hipStreamSynchronize(g_stream));        // (the kernels of an earlier enqueue-only call may still read the weights)
        HIPCHK(hipMemcpy(L.d_wq, wq.data(), sizeof(double) * wq.size(), hipMemcpyHostToDevice));
        L.wq = wq;
    }
    CommPattern* cp = nullptr;
    if (jm_pattern_of(level, S.J.lStart, nS, who, &cp)) return 1;
    if (cp && (!cp->sends.empty() || !cp->recvs.empty())) return fail("%s: the level exchanges halos with other ranks (one rank only)", who);
    if (cp && jm_acc_lists(cp)) return 1;
    for (size_t q = 0; q < L.barYs.size(); ++q)
        if (L.barYs[q]) HIPCHK(hipMemsetAsync(L.barYs[q], 0, L.barYsBytes[q], g_stream));
    // (from here on every exit goes through jf_finish, which gives the slab back after an error)
    int rc = wd_prepare(who, level, S, sync);
    if (!rc) {
        const KParams kp = res_kparams(level, S.resFlags);
        const size_t nt = (size_t)L.barSlots + 1;
        JacSpec C = S.J;
        C.ca = 1; C.cb = WI_CM; C.cc = WI_CM * WI_CM; C.cn = WI_NCOL; C.cm = WI_CM;
        for (int l = S.J.lStart; l < S.J.lStart + nS && !rc; ++l)
            for (int col = 0; col < WI_NCOL && !rc; ++col) {
                for_level(level, [&](Block* b) {
                    ad_launch_seed_closures(b->v, g_ad[b].v, l, col, C, kp, g_stream, false);
                    return 0;
                });
                rc = wd_front_enqueue(level, S, kp, F != nullptr);
                if (rc) break;
                if (F) ad_launch_flowint_bar(g_ad_tab, L.d_faces, nface, L.maxOwned, *F, L.d_wq, nRhs, L.nOwned, L.d_g, g_stream);
                else ad_launch_wallint_bar(g_ad_tab, L.d_faces, nface, L.maxOwned, P, kp, L.d_wq, nRhs, L.nOwned, L.d_g, g_stream);
                launch_wallint_credit(L.d_faces, nface, L.maxBox, L.barTab, (long)nt, nRhs, l - S.J.lStart, col, L.d_g, L.nOwned, g_stream);
            }
        for (int r = 0; r < nRhs && !rc; ++r) {
            // the reverse exchange of jacobian_mult: every halo with a donor is added to it in the fixed order of the donor's list
            if (cp) launch_jac_halo_accumulate(L.barTab + r * nt, cp->acc[0], nS, nullptr, 0, g_stream);
            launch_jm_gather(L.barTab + r * nt, L.barSlots, L.barNx, L.barNy, L.barNz, nS, d_wbar + r * ld, g_stream);
        }
    }
    return jf_finish(rc);
}

static int wd_bwd(const char* who, int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                  const double* outBar, int nRhs, double* wbar, long n, long ld, bool dev, bool flow = false)
{
    if (need_ready()) return 1;
    if (!outBar || !wbar) return fail("%s: %s is NULL", who, !outBar ? "outBar" : "wbar");
    if (nRhs < 1 || nRhs > ADFLOW_GPU_MAX_NVEC) return fail("%s: nRhs = %d; one call takes 1 to %d weight sets", who, nRhs, ADFLOW_GPU_MAX_NVEC);
    if (wd_check_flags(who, flags)) return 1;
    JfSetup S;
    if (jf_check(who, level, flags, outBar, wbar, n, &S)) return 1;
    if (ld < n) return fail("%s: ld = %ld, but a column holds n = %ld entries (ld >= n)", who, ld, n);
    if (flow) {
        // (the flow entry refuses before its record exists, so that the refusal leaves nothing allocated; the wall entry refuses
        //  where it always did, in wd_bwd_enqueue)
        CommPattern* cp = nullptr;
        if (jm_pattern_of(level, S.J.lStart, S.J.nState, who, &cp)) return 1;
        if (cp && (!cp->sends.empty() || !cp->recvs.empty())) return fail("%s: the level exchanges halos with other ranks (one rank only)", who);
    }
    WiPar P;
    FiPar FP;
    const FiPar* F = flow ? &FP : nullptr;
    WiLevel* L;
    int nG;
    if (flow ? fi_setup(who, level, par, nGroups, famLists, ldFam, &FP, &L, &nG)
             : wi_setup(who, level, par, nGroups, famLists, ldFam, false, &P, &L, &nG))
        return 1;
    // the weight of quantity q of subface f in set r: outBar summed over the groups the subface belongs to
    static const int entryOf[WI_NQ] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 44, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 17, 63};
    static const int flowEntryOf[FI_NQ] = {18, 19, 20, 21, 31, 35, 36, 38, 39, 40, 41, 42, 43, 59, 37, 47, 48, 0, 1, 2, 22, 23, 24,
                                           25, 26, 27, 28, 29, 30, 50, 51, 52, 53, 54, 55, 56, 57, 58};
    const int* eo = flow ? flowEntryOf : entryOf;
    const int nq = L->nq, nqSum = flow ? FI_NQ : WI_YPLUS;
    const int nface = (int)L->faces.size();
    std::vector<double> wq((size_t)nRhs * nface * nq, 0.0);
    for (int r = 0; r < nRhs; ++r)
        for (int g = 0; g < nG; ++g) {
            const double* ob = outBar + ((size_t)r * nG + g) * ADFLOW_WALLINT_STRIDE;
            if (!flow && (ob[17] != 0.0 || ob[63] != 0.0))
                return fail("%s: weight set %d, group %d: entry %d (%s) has no derivative, its weight must be zero", who, r + 1, g + 1,
                            ob[17] != 0.0 ? 17 : 63, ob[17] != 0.0 ? "yplusMax" : "the minimum of Cp");
            for (int f = 0; f < nface; ++f) {
                if (!L->member[(size_t)g * nface + f]) continue;
                for (int q = 0; q < nqSum; ++q) wq[((size_t)r * nface + f) * nq + q] += ob[eo[q]];
            }
        }
    if (dev) {
        if (wd_bwd_enqueue(who, level, S, P, F, *L, wq, nRhs, wbar, n, ld, !g_async)) return 1;
        return sync_and_check();
    }
    DevBuf buf;
    HIPCHK(hipMalloc(&buf.p, sizeof(double) * std::max<size_t>(1, (size_t)nRhs * n)));
    const Stage s{n, (double*)buf.p};
    if (wd_bwd_enqueue(who, level, S, P, F, *L, wq, nRhs, s[0], n, n, false)) return 1;
    return stage_out_columns(s, wbar, ld, 0, nRhs) || s.done();
}

int adflow_gpu_wall_integrate_bwd(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                  const double* outBar, int nRhs, double* wbar, long n, long ld)
{
    return wd_bwd("wall_integrate_bwd", level, flags, par, nGroups, famLists, ldFam, outBar, nRhs, wbar, n, ld, false);
}

int adflow_gpu_wall_integrate_bwd_dev(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                      const double* outBar, int nRhs, double* d_wbar, long n, long ld)
{
    return wd_bwd("wall_integrate_bwd_dev", level, flags, par, nGroups, famLists, ldFam, outBar, nRhs, d_wbar, n, ld, true);
}

// the same two entries for the in- and outflow subfaces (flowIntegrationFace_d / _b): the record of the flow subfaces, the dual flow
// boundary conditions as the only front
int adflow_gpu_flow_integrate_fwd(int level, unsigned flags, const double* x, long n, const double* par, int nGroups, const int32_t* famLists,
                                  int ldFam, double* out, double* outDot)
{
    return wd_fwd("flow_integrate_fwd", level, flags, x, n, par, nGroups, famLists, ldFam, out, outDot, false, true);
}

int adflow_gpu_flow_integrate_fwd_dev(int level, unsigned flags, const double* d_x, long n, const double* par, int nGroups,
                                      const int32_t* famLists, int ldFam, double* d_out, double* d_outDot)
{
    return wd_fwd("flow_integrate_fwd_dev", level, flags, d_x, n, par, nGroups, famLists, ldFam, d_out, d_outDot, true, true);
}

int adflow_gpu_flow_integrate_bwd(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                  const double* outBar, int nRhs, double* wbar, long n, long ld)
{
    return wd_bwd("flow_integrate_bwd", level, flags, par, nGroups, famLists, ldFam, outBar, nRhs, wbar, n, ld, false, true);
}

int adflow_gpu_flow_integrate_bwd_dev(int level, unsigned flags, const double* par, int nGroups, const int32_t* famLists, int ldFam,
                                      const double* outBar, int nRhs, double* d_wbar, long n, long ld)
{
    return wd_bwd("flow_integrate_bwd_dev", level, flags, par, nGroups, famLists, ldFam, outBar, nRhs, d_wbar, n, ld, true, true);
}

// nvec right-hand sides on the assembled matrix with the selected factor, in lock-step: every iteration is ONE application of M^-1
// and ONE product for all columns, every launch of the Gram-Schmidt chain carries all columns (each with its own partial sums, added
// in the order of gm_solve), and one download and one synchronise bring the Hessenberg columns of all of them.  The host keeps a GmLsq,
// a tolerance and a count per column, and a column ends exactly where gm_solve would end it; from then on its basis vectors are zeros
// (M^-1 0 = 0, J 0 = 0: nothing that is not finite), its x is not touched (GmCoef: a = 0, b = 1), and the residual evaluation at the
// next restart boundary -- which the columns that go on need anyway -- gives its true residual norm.
// Work space: (restart + 3) nvec vectors; basis vector j of column c at V + (j nvec + c) n.
static int gm_solve_multi(const char* who, int level, int transpose, int nvec, const double* d_B, long ldb, double* d_X, long ldx, long n,
                          int restart, int maxIts, double rtol, double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    const int m = std::max(1, std::min(restart, std::max(maxIts, 1)));
    DevBuf buf;
    const size_t nv = (size_t)(m + 3) * nvec * n, nred = (size_t)nvec * (2 * GM_PARTS + m + 2);
    if (hipMalloc(&buf.p, (nv + nred) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        buf.p = nullptr;
        return fail("%s: cannot allocate %zu bytes for the (restart + 3) x nvec = %d x %d vectors of %ld entries; nothing is held", who,
                    (nv + nred) * sizeof(double), m + 3, nvec, n);
    }
    const size_t cn = (size_t)nvec * n;                  // one vector of every column
    double* V = (double*)buf.p;
    double *zt = V + (size_t)(m + 1) * cn, *tv = zt + cn, *red = tv + cn, *P[2] = {red, red + (size_t)nvec * GM_PARTS},
           *dH = red + (size_t)2 * nvec * GM_PARTS;     // dH[i nvec + c]: entry i of the Hessenberg column of column c
    std::vector<double> H((size_t)(m + 2) * nvec);
    hipStream_t s = g_stream;
    auto norms = [&](const double* a, long lda, double* out) -> int {      // out[c] = ||a_c||
        launch_gm_mgs_multi(const_cast<double*>(a), nullptr, nullptr, nullptr, P[0], nullptr, n, lda, nvec, s);
        launch_gm_sum_multi(P[0], n, dH, nvec, s);
        HIPCHK(hipMemcpyAsync(H.data(), dH, sizeof(double) * nvec, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int c = 0; c < nvec; ++c) out[c] = (H[c] == H[c]) ? sqrt(std::max(H[c], 0.0)) : H[c];      // NaN stays NaN
        return 0;
    };
    auto pc = [&](const double* r, double* z) { return pc_apply_multi_enqueue(who, transpose, nvec, r, n, z, n, s); };
    GmCoef all;
    for (int c = 0; c < GM_MAXV; ++c) { all.a[c] = 1.0; all.b[c] = -1.0; }
    enum { RUNNING, STOPPED, DONE };  // STOPPED: ended inside the cycle, its true residual comes with the next residual evaluation
    struct Col { GmLsq q; int state = RUNNING, total = 0, k = 0; double tol = 0.0, res = 0.0; explicit Col(int m) : q(m) {} };
    std::vector<Col> col(nvec, Col(m));
    std::vector<double> nrm(nvec);
    if (norms(d_B, ldb, nrm.data())) return 1;
    for (int c = 0; c < nvec; ++c) {
        if (!(nrm[c] == nrm[c])) return fail("%s: the right-hand side of column %d is not finite", who, c);
        col[c].tol = std::max(rtol * nrm[c], atol);
    }
    if (!useGuess)
        for (int c = 0; c < nvec; ++c) HIPCHK(hipMemsetAsync(d_X + c * ldx, 0, sizeof(double) * n, s));
    bool first = true, zeroX = !useGuess;
    for (;;) {
        // r = b - A x of every column: the start of a cycle for the columns that run, the true residual for those that stopped
        if (zeroX) {
            for (int c = 0; c < nvec; ++c) HIPCHK(hipMemcpyAsync(V + (size_t)c * n, d_B + c * ldb, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
        } else {
            if (jm_mult_multi_enqueue(level, transpose, nvec, d_X, ldx, V, n)) return 1;
            launch_gm_axpby_multi(V, n, d_B, ldb, all, n, nvec, s);
        }
        if (norms(V, n, nrm.data())) return 1;
        GmCoef k;
        int running = 0;
        for (int c = 0; c < nvec; ++c) {
            Col& q = col[c];
            if (first && rnorm0) rnorm0[c] = nrm[c];
            k.a[c] = 0.0; k.b[c] = 1.0;
            if (q.state == DONE) continue;
            q.res = nrm[c];
            if (q.state == STOPPED) { q.state = DONE; continue; }
            if (!(nrm[c] == nrm[c])) return fail("%s: the residual of column %d is not finite after %d iterations", who, c, q.total);
            if (nrm[c] <= q.tol || q.total >= maxIts) { q.state = DONE; continue; }
            k.a[c] = 1.0 / nrm[c]; k.b[c] = 0.0;
            q.q.start(nrm[c]);
            q.k = 0;
            ++running;
        }
        first = false;
        if (!running) break;
        for (int c = 0; c < nvec; ++c)
            if (col[c].state == DONE) HIPCHK(hipMemsetAsync(V + (size_t)c * n, 0, sizeof(double) * n, s));
        launch_gm_axpby_multi(V, n, V, n, k, n, nvec, s);
        std::vector<char> inCycle(nvec);
        for (int c = 0; c < nvec; ++c) inCycle[c] = col[c].state == RUNNING;
        int kmax = 0;
        for (int j = 0; j < m && running; ++j) {
            double* w = V + (size_t)(j + 1) * cn;
            if (pc(V + (size_t)j * cn, zt)) return 1;
            if (jm_mult_multi_enqueue(level, transpose, nvec, zt, n, w, n)) return 1;
            launch_gm_mgs_multi(w, nullptr, nullptr, V, P[0], nullptr, n, n, nvec, s);
            for (int i = 1; i <= j; ++i)
                launch_gm_mgs_multi(w, V + (size_t)(i - 1) * cn, P[(i - 1) & 1], V + (size_t)i * cn, P[i & 1], dH + (size_t)(i - 1) * nvec, n, n,
                                    nvec, s);
            launch_gm_mgs_multi(w, V + (size_t)j * cn, P[j & 1], nullptr, P[(j + 1) & 1], dH + (size_t)j * nvec, n, n, nvec, s);
            launch_gm_sum_multi(P[(j + 1) & 1], n, dH + (size_t)(j + 1) * nvec, nvec, s);
            HIPCHK(hipMemcpyAsync(H.data(), dH, sizeof(double) * (j + 2) * nvec, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            kmax = j + 1;
            for (int c = 0; c < nvec; ++c) {
                Col& q = col[c];
                k.a[c] = 0.0; k.b[c] = 1.0;
                if (q.state != RUNNING) continue;
                const double h2 = H[(size_t)(j + 1) * nvec + c], hn = sqrt(std::max(h2, 0.0));
                if (!(h2 == h2)) return fail("%s: the Krylov vector of iteration %d of column %d is not finite", who, q.total + 1, c);
                q.res = q.q.column(H.data() + c, nvec, j, hn);
                ++q.total;
                q.k = j + 1;
                if (q.res <= q.tol || q.total >= maxIts || !(hn > 0.0)) {
                    q.state = STOPPED;
                    --running;
                    HIPCHK(hipMemsetAsync(w + (size_t)c * n, 0, sizeof(double) * n, s));
                } else {
                    k.a[c] = 1.0 / hn; k.b[c] = 0.0;
                }
            }
            if (running) launch_gm_axpby_multi(w, n, w, n, k, n, nvec, s);
        }
        // x += M^-1 (V y) for the columns of this cycle, each with the coefficients of its own k basis vectors
        for (int c = 0; c < nvec; ++c)
            if (inCycle[c]) col[c].q.solve(col[c].k);
        for (int i = 0; i < kmax; ++i) {
            for (int c = 0; c < nvec; ++c) {
                const bool on = inCycle[c] && i < col[c].k;
                k.a[c] = on ? col[c].q.y[i] : 0.0;
                k.b[c] = (i == 0) ? 0.0 : 1.0;               // i == 0 sets every column of tv: zero where no cycle ran
            }
            launch_gm_axpby_multi(tv, n, V + (size_t)i * cn, n, k, n, nvec, s);
        }
        if (pc(tv, zt)) return 1;
        for (int c = 0; c < nvec; ++c) { k.a[c] = inCycle[c] ? 1.0 : 0.0; k.b[c] = 1.0; }
        launch_gm_axpby_multi(d_X, ldx, zt, n, k, n, nvec, s);
        zeroX = false;
    }
    for (int c = 0; c < nvec; ++c) {
        if (its) its[c] = col[c].total;
        if (rnorm) rnorm[c] = col[c].res;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int gm_check_multi(int level, int nvec, const double* B, long ldb, const double* X, long ldx, long n, int restart, int maxIts,
                          double rtol, double atol)
{
    const char* who = "gmres_solve_multi";
    if (gm_check_ranks(who, "adflow_gpu_jacobian_mult_multi_dev")) return 1;
    if (multi_check(who, nvec, B, ldb, X, ldx, n)) return 1;
    if (!g_jac_valid) return fail("%s: no assembled Jacobian (call adflow_gpu_fd_jacobian first)", who);
    if (pc_check(who, level, B, X, n, false)) return 1;
    if (g_jac.nState != pc_sel().nState)
        return fail("%s: the factor was set up for nState = %d, the assembled matrix has nState = %d", who, pc_sel().nState, g_jac.nState);
    if (jm_check(level, B, X, n, who)) return 1;
    if (n != pc_sel().ncell * pc_sel().nState) return fail("%s: n=%ld but the factor has %ld rows", who, n, pc_sel().ncell * pc_sel().nState);
    return gm_check_caps(who, restart, maxIts, rtol, atol);
}

int adflow_gpu_gmres_solve_multi_dev(int level, int transpose, int nvec, const double* d_B, long ldb, double* d_X, long ldx, long n,
                                     int restart, int maxIts, double rtol, double atol, int useGuess, int* its, double* rnorm0,
                                     double* rnorm)
{
    if (gm_check_multi(level, nvec, d_B, ldb, d_X, ldx, n, restart, maxIts, rtol, atol)) return 1;
    if (nvec == 1) {                   // one column: the single solver, to the bit
        const GmOperator op = [=](const double* v, double* y) { return jm_mult_enqueue(level, transpose, v, y); };
        return gm_solve("gmres_solve_multi", op, transpose, d_B, d_X, n, restart, maxIts, rtol, atol, useGuess, its, rnorm0, rnorm);
    }
    return gm_solve_multi("gmres_solve_multi", level, transpose, nvec, d_B, ldb, d_X, ldx, n, restart, maxIts, rtol, atol, useGuess, its,
                          rnorm0, rnorm);
}

int adflow_gpu_gmres_solve_multi(int level, int transpose, int nvec, const double* B, long ldb, double* X, long ldx, long n, int restart,
                                 int maxIts, double rtol, double atol, int useGuess, int* its, double* rnorm0, double* rnorm)
{
    if (gm_check_multi(level, nvec, B, ldb, X, ldx, n, restart, maxIts, rtol, atol)) return 1;
    DevBuf buf;                        // B and X of this call side by side, not g_vec_dev
    if (hipMalloc(&buf.p, sizeof(double) * 2 * nvec * n) != hipSuccess) {
        (void)hipGetLastError();
        buf.p = nullptr;
        return fail("gmres_solve_multi: cannot allocate %zu bytes for %d right-hand sides and solutions of %ld entries",
                    sizeof(double) * 2 * nvec * n, nvec, n);
    }
    const Stage s{n, (double*)buf.p};
    if (stage_in_columns(s, 0, B, ldb, nvec) || (useGuess && stage_in_columns(s, nvec, X, ldx, nvec))) return 1;
    return adflow_gpu_gmres_solve_multi_dev(level, transpose, nvec, s[0], n, s[nvec], n, n, restart, maxIts, rtol, atol, useGuess, its,
                                            rnorm0, rnorm) ||
           stage_out_columns(s, X, ldx, nvec, nvec) || s.done();
}

// ---- the approximate Newton-Krylov step (kernels_ank.hip) -------------------------------------------------------------------------
// ANKStep (NKSolvers.F90:3629-4112) up to the linear solve and the step limiter: setWANK / setRVecANK, computeTimeStepMat for
// ANK_charTimeStepType = 'None', the ILU(0) of dRdwPre + timeStepMat, the matrix-free operator of FormFunction_mf under MatMFFD,
// KSPSolve and physicalityCheckANK.  Vectors carry nState = nw (ADFLOW_ANK_COUPLED) or 5 variables per owned level-1 cell.
// ANKTurbSolveKSP (:3337-3627) the same way with ADFLOW_ANK_TURB: one entry per cell, FormFunction_mf_turb, physicalityCheckANKTurb.
// The flow kind (nState 5 or nw) and the turbulence kind (nState 1) each keep a T and a base; the flag selects one on every entry.
namespace {
struct AnkKind {
    bool haveT = false;                // the pseudo-time term: flow tsm[q N + m], q = 0 dtInv, 1 rho, 2..4 u, v, w; turbulence dtInv only
    int tLevel = 0, tNState = 0;
    long tCells = 0;
    double turbDiag = 0.0;
    double* tsm = nullptr;
    bool haveBase = false;             // the base of the matrix-free operator: w and r0 = R(w)
    int nState = 0;
    unsigned flags = 0;
    long ncell = 0;
    double *w0 = nullptr, *r0 = nullptr;
    size_t bytesT = 0, bytesBase = 0;
};
struct AnkState {
    AnkKind kind[2];                   // 0 flow, 1 turbulence
    int last = 0;                      // the kind of the base set last: adflow_gpu_ank_mult / _solve / _last_h act on it
    double* red = nullptr;             // ANK_RED doubles: partial sums, partial minima and the scalars (the ANK_RED_.. layout of internal.h)
    double* part = nullptr;            // the partial sums of adflow_gpu_ank_unsteady_res, one per workgroup
    long partCap = 0;
    size_t bytesRed = 0, bytesPart = 0;
};
AnkState g_ank;
const unsigned ANK_RES_FLAGS = ADFLOW_RES_DISS_APPROX | ADFLOW_RES_VISC_APPROX | ADFLOW_RES_UPWIND_FIRST_ORDER | ADFLOW_RES_APPROX_SA |
                               ADFLOW_RES_TURB_FIRST_ORDER;
const unsigned ANK_KIND_FLAGS = ADFLOW_ANK_COUPLED | ADFLOW_ANK_TURB;
static bool ank_is_turb(unsigned flags) { return (flags & ADFLOW_ANK_TURB) != 0; }
static AnkKind& ank_kind(unsigned flags) { return g_ank.kind[ank_is_turb(flags) ? 1 : 0]; }
static AnkKind& ank_last() { return g_ank.kind[g_ank.last]; }
static double* ank_scal(AnkScal q) { return g_ank.red + ANK_RED_SCAL + q; }   // a scalar of the buffer; ank_scal(ANK_H) is `hdev`
}  // namespace

static int64_t ank_release()
{
    int64_t n = (int64_t)(g_ank.bytesRed + g_ank.bytesPart);
    for (AnkKind& k : g_ank.kind) {
        n += (int64_t)(k.bytesT + k.bytesBase);
        if (k.tsm) (void)hipFree(k.tsm);
        if (k.w0) (void)hipFree(k.w0);
    }
    if (g_ank.red) (void)hipFree(g_ank.red);
    if (g_ank.part) (void)hipFree(g_ank.part);
    g_ank = AnkState();
    return n;
}

int adflow_gpu_ank_release(int64_t* bytes)
{
    if (g_stream) HIPCHK(hipStreamSynchronize(g_stream));
    const int64_t n = ank_release();
    if (bytes) *bytes = n;
    return 0;
}

static int ank_red()
{
    if (g_ank.red) return 0;
    HIPCHK(hipMalloc((void**)&g_ank.red, ANK_RED * sizeof(double)));
    HIPCHK(hipMemsetAsync(g_ank.red, 0, ANK_RED * sizeof(double), g_stream));
    g_ank.bytesRed = ANK_RED * sizeof(double);
    return 0;
}

// owned cells and nState of the vectors of `level` for these flags
static int ank_dims(const char* who, int level, unsigned flags, long* cells, int* nS)
{
    if (need_ready()) return 1;
    if (flags & ~(ANK_KIND_FLAGS | ANK_RES_FLAGS))
        return fail("%s: flags = %u; accepted are ADFLOW_ANK_COUPLED or ADFLOW_ANK_TURB and ADFLOW_RES_DISS_APPROX / _VISC_APPROX / "
                    "_UPWIND_FIRST_ORDER / _APPROX_SA / _TURB_FIRST_ORDER", who, flags);
    if ((flags & ANK_KIND_FLAGS) == ANK_KIND_FLAGS)
        return fail("%s: flags = %u; ADFLOW_ANK_TURB (the turbulence KSP of the decoupled step) excludes ADFLOW_ANK_COUPLED", who, flags);
    if (ank_is_turb(flags) && g_opts.equations != ADFLOW_RANS) return fail("%s: ADFLOW_ANK_TURB needs the RANS equations", who);
    long n = 0;
    int nw = 0;
    int rc = for_level(level, [&](Block* b) {
        if (nw && nw != b->v.nw) return fail("%s: the blocks of level %d carry different nw", who, level);
        nw = b->v.nw;
        n += (long)b->v.nx * b->v.ny * b->v.nz;
        return 0;
    });
    if (rc) return rc;
    if (!n) return fail("no block registered on level %d", level);
    if (ank_is_turb(flags) && nw < 6) return fail("%s: RANS/SA needs nw = 6 (block has %d)", who, nw);
    *cells = n;
    *nS = ank_is_turb(flags) ? 1 : (flags & ADFLOW_ANK_COUPLED) ? nw : 5;
    return 0;
}

static int ank_vec_check(const char* who, const double* a, const double* b, long n, unsigned flags, long* cells, int* nS)
{
    if (ank_dims(who, 1, flags, cells, nS)) return 1;
    if (!a || !b) return fail("%s: a vector is NULL", who);
    if (n != *cells * *nS)
        return fail("%s: n=%ld but the level-1 blocks hold %ld entries (nState = %d x %ld owned cells)", who, n, *cells * *nS, *nS, *cells);
    return 0;
}

// turb: nuTilde only (nS = 1); withClosures then means the eddy viscosity of the cell and nothing else (the flow variables stand)
static int ank_set_w_enqueue(const double* d_w, int nS, bool withClosures, const double* d_v = nullptr, const double* hdev = nullptr,
                             bool turb = false)
{
    LevelTab t;
    if (level_tab(1, &t)) return 1;
    if (turb) {
        // no flow variable moves: the sensor and the energy / pressure consistency of the blocks stand as they are
        KParams kp = make_kparams(1, 1.0, 0);
        launch_ank_set_w_turb(t.tab, t.n, t.nx, t.ny, t.nz, d_w, d_v, hdev, withClosures ? &kp : nullptr, g_stream);
        return 0;
    }
    if (withClosures) {
        KParams kp = make_kparams(1, 1.0, 0);
        if (floor_flag_clear()) return 1;
        launch_ank_set_w(t.tab, t.n, t.nx, t.ny, t.nz, nS, d_w, d_v, hdev, &kp, g_floor_flag_dev, g_stream);
    } else
        launch_ank_set_w(t.tab, t.n, t.nx, t.ny, t.nz, nS, d_w, d_v, hdev, nullptr, nullptr, g_stream);
    return flow_state_written();
}

// blocketteRes(useDissApprox, useViscApprox, useTurbRes = ANK_coupled, useStoreWall = F) behind a state write that did the closures;
// ADFLOW_ANK_TURB: blocketteRes(useFlowRes = F, useStoreWall = F) behind a turbulence state write that re-formed the eddy viscosity.
// closures: the evaluation forms them itself (the state came from adflow_gpu_ank_set_w)
static int ank_res_enqueue(unsigned flags, bool closures = false)
{
    unsigned f = ADFLOW_RES_HALO | (flags & ANK_RES_FLAGS) | (closures ? ADFLOW_RES_CLOSURES : 0u);
    if (ank_is_turb(flags)) return block_res_enqueue(1, f | ADFLOW_RES_TURB);
    f |= ADFLOW_RES_FLOW;
    if ((flags & ADFLOW_ANK_COUPLED) && g_opts.equations == ADFLOW_RANS) f |= ADFLOW_RES_TURB;
    if (closures) return block_res_enqueue(1, f);
    g_etot_flag_level = 1;      // the owned energy is computeEtot(p) already wherever p kept its value
    const int rc = block_res_enqueue(1, f);
    g_etot_flag_level = 0;
    return rc;
}

static int ank_get_r_enqueue(double* d_r, int nS, bool turb = false)
{
    LevelTab t;
    if (level_tab(1, &t)) return 1;
    if (turb) launch_ank_get_r_turb(t.tab, t.n, t.nx, t.ny, t.nz, d_r, g_opts.turbResScale, g_stream);
    else launch_ank_get_r(t.tab, t.n, t.nx, t.ny, t.nz, nS, d_r, g_opts.turbResScale, g_stream);
    return 0;
}

int adflow_gpu_ank_set_w_dev(const double* d_w, long n, unsigned flags)
{
    long cells; int nS;
    if (ank_vec_check("ank_set_w", d_w, d_w, n, flags, &cells, &nS)) return 1;
    if (ank_set_w_enqueue(d_w, nS, false, nullptr, nullptr, ank_is_turb(flags))) return 1;
    return sync_and_check();
}

int adflow_gpu_ank_set_w(const double* w, long n, unsigned flags)
{
    long cells; int nS;
    Stage s;
    return ank_vec_check("ank_set_w", w, w, n, flags, &cells, &nS) || stage_open(&s, n, 1) || s.in(0, w) ||
           ank_set_w_enqueue(s[0], nS, false, nullptr, nullptr, ank_is_turb(flags)) || s.done();
}

int adflow_gpu_ank_get_r_dev(double* d_r, long n, unsigned flags)
{
    long cells; int nS;
    if (ank_vec_check("ank_get_r", d_r, d_r, n, flags, &cells, &nS)) return 1;
    if (ank_get_r_enqueue(d_r, nS, ank_is_turb(flags))) return 1;
    return sync_and_check();
}

int adflow_gpu_ank_get_r(double* r, long n, unsigned flags)
{
    long cells; int nS;
    Stage s;
    return ank_vec_check("ank_get_r", r, r, n, flags, &cells, &nS) || stage_open(&s, n, 1) || ank_get_r_enqueue(s[0], nS, ank_is_turb(flags)) ||
           s.out(r, 0) || s.done();
}

int adflow_gpu_ank_time_step(int level, double cfl, double turbCFLScale, unsigned flags)
{
    long cells; int nS;
    if (ank_dims("ank_time_step", level, flags & ANK_KIND_FLAGS, &cells, &nS)) return 1;
    if (!(cfl > 0.0)) return fail("ank_time_step: cfl = %g", cfl);
    const bool turb = ank_is_turb(flags);
    if ((nS > 5 || turb) && !(turbCFLScale > 0.0)) return fail("ank_time_step: turbCFLScale = %g", turbCFLScale);
    AnkKind& K = ank_kind(flags);
    if (K.tsm && K.tCells != cells) {
        HIPCHK(hipStreamSynchronize(g_stream));
        (void)hipFree(K.tsm);
        K.tsm = nullptr;
        K.bytesT = 0;
    }
    K.haveT = false;
    const int nq = turb ? 1 : 5;
    if (!K.tsm) {
        HIPCHK(hipMalloc((void**)&K.tsm, sizeof(double) * nq * cells));
        K.bytesT = sizeof(double) * nq * cells;
    }
    LevelTab t;
    if (level_tab(level, &t)) return 1;
    if (turb) launch_ank_time_step_turb(t.tab, t.n, t.nx, t.ny, t.nz, cfl, K.tsm, g_stream);
    else launch_ank_time_step(t.tab, t.n, t.nx, t.ny, t.nz, cfl, K.tsm, cells, g_stream);
    K.tLevel = level; K.tNState = nS; K.tCells = cells;
    K.turbDiag = (nS > 5 || turb) ? g_opts.turbResScale / turbCFLScale : 0.0;
    K.haveT = true;
    return sync_and_check();
}

static int ank_download_time_step(int nn, double* blocks, unsigned flags)
{
    if (need_ready()) return 1;
    if (flags & ~ADFLOW_ANK_TURB) return fail("ank_download_time_step: flags = %u; accepted is ADFLOW_ANK_TURB", flags);
    const bool turb = ank_is_turb(flags);
    const AnkKind& K = ank_kind(flags);
    if (!K.haveT)
        return fail("ank_download_time_step: no pseudo-time term%s (call adflow_gpu_ank_time_step first)", turb ? " of the turbulence KSP" : "");
    if (!blocks) return fail("ank_download_time_step: blocks is NULL");
    Block* b = find_block(nn, K.tLevel, 1);
    if (!b) return fail("block (%d,%d,1) not registered", nn, K.tLevel);
    long off = 0;
    for (auto& kv : g_blocks)
        if (std::get<0>(kv.first) == K.tLevel && std::get<2>(kv.first) < nn) off += (long)kv.second->v.nx * kv.second->v.ny * kv.second->v.nz;
    const long nc = (long)b->v.nx * b->v.ny * b->v.nz, N = K.tCells;
    const int nS = K.tNState, nq = turb ? 1 : 5;
    std::vector<double> h((size_t)nq * nc);
    HIPCHK(hipStreamSynchronize(g_stream));
    for (int q = 0; q < nq; ++q) HIPCHK(hipMemcpy(h.data() + (size_t)q * nc, K.tsm + (size_t)q * N + off, sizeof(double) * nc, hipMemcpyDeviceToHost));
    if (turb) {
        for (long c = 0; c < nc; ++c) blocks[c] = h[c] * K.turbDiag;
        return 0;
    }
    memset(blocks, 0, sizeof(double) * nS * nS * nc);
    for (long c = 0; c < nc; ++c) {
        double* B = blocks + (size_t)c * nS * nS;      // B[ll + l nS] = T(ll, l)
        const double dtInv = h[c], rho = h[nc + c];
        B[0] = dtInv;
        B[4 + 4 * nS] = dtInv;
        for (int l = 1; l < 4; ++l) {
            B[l] = dtInv * h[(size_t)(l + 1) * nc + c];
            B[l + l * nS] = dtInv * rho;
        }
        if (nS > 5) B[5 + 5 * nS] = dtInv * K.turbDiag;
    }
    return 0;
}

int adflow_gpu_ank_download_time_step(int nn, double* blocks) { return ank_download_time_step(nn, blocks, 0u); }
int adflow_gpu_ank_download_time_step_turb(int nn, double* blocks, unsigned flags) { return ank_download_time_step(nn, blocks, flags); }

int adflow_gpu_ank_pc_setup(int level)
{
    if (pc_setup_check("ank_pc_setup", level)) return 1;
    // an ADFLOW_JAC_TURB_ONLY matrix takes the turbulence T (FormJacobianANKTurb), every other the flow T (FormJacobianANK)
    const bool turb = g_jac.nState == 1;
    const AnkKind& K = g_ank.kind[turb ? 1 : 0];
    if (!K.haveT)
        return fail("ank_pc_setup: no pseudo-time term%s (call adflow_gpu_ank_time_step first)",
                    turb ? " of the turbulence KSP, which the ADFLOW_JAC_TURB_ONLY matrix takes" : "");
    if (K.tLevel != level) return fail("ank_pc_setup: level %d is not the level of the pseudo-time term (%d)", level, K.tLevel);
    if (K.tNState != g_jac.nState)
        return fail("ank_pc_setup: the pseudo-time term was formed for nState = %d, the assembled matrix has nState = %d", K.tNState,
                    g_jac.nState);
    return pc_setup_selected(level, K.tsm, K.turbDiag);
}

static int ank_set_base_enqueue(const double* d_w, long n, long cells, int nS, unsigned flags)
{
    if (ank_red()) return 1;
    AnkKind& K = ank_kind(flags);
    const bool turb = ank_is_turb(flags);
    if (K.w0 && (K.ncell != cells || K.nState != nS)) {
        HIPCHK(hipStreamSynchronize(g_stream));
        (void)hipFree(K.w0);
        K.w0 = K.r0 = nullptr;
        K.bytesBase = 0;
    }
    K.haveBase = false;
    if (!K.w0) {
        HIPCHK(hipMalloc((void**)&K.w0, sizeof(double) * 2 * n));
        K.r0 = K.w0 + n;
        K.bytesBase = sizeof(double) * 2 * n;
    }
    K.ncell = cells; K.nState = nS; K.flags = flags;
    g_ank.last = turb ? 1 : 0;
    HIPCHK(hipMemcpyAsync(K.w0, d_w, sizeof(double) * n, hipMemcpyDeviceToDevice, g_stream));
    if (ank_set_w_enqueue(K.w0, nS, true, nullptr, nullptr, turb)) return 1;
    if (ank_res_enqueue(flags)) return 1;
    if (ank_get_r_enqueue(K.r0, nS, turb)) return 1;
    K.haveBase = true;
    return 0;
}

int adflow_gpu_ank_set_base_dev(const double* d_w, long n, unsigned flags)
{
    long cells; int nS;
    if (ank_vec_check("ank_set_base", d_w, d_w, n, flags, &cells, &nS)) return 1;
    if (ank_set_base_enqueue(d_w, n, cells, nS, flags)) return 1;
    return sync_and_check();
}

int adflow_gpu_ank_set_base(const double* w, long n, unsigned flags)
{
    long cells; int nS;
    Stage s;
    return ank_vec_check("ank_set_base", w, w, n, flags, &cells, &nS) || stage_open(&s, n, 1) || s.in(0, w) ||
           ank_set_base_enqueue(s[0], n, cells, nS, flags) || s.done();
}

static int ank_mult_check(const char* who, const double* v, const double* y, long n)
{
    if (need_ready()) return 1;
    const AnkKind& K = ank_last();
    if (!K.haveBase) return fail("%s: no base state (call adflow_gpu_ank_set_base first)", who);
    if (!K.haveT)
        return fail("%s: no pseudo-time term%s (call adflow_gpu_ank_time_step first)", who, g_ank.last ? " of the turbulence KSP" : "");
    if (K.tLevel != 1 || K.tNState != K.nState || K.tCells != K.ncell)
        return fail("%s: the pseudo-time term was formed for nState = %d on level %d, the base state has nState = %d on level 1", who,
                    K.tNState, K.tLevel, K.nState);
    if (!v || !y) return fail("%s: a vector is NULL", who);
    if (v == y) return fail("%s: input and result are the same vector (not done in place)", who);
    if (n != K.ncell * K.nState)
        return fail("%s: n=%ld but the base state has %ld rows (nState = %d x %ld owned cells)", who, n, K.ncell * K.nState,
                    K.nState, K.ncell);
    return 0;
}

// y = (R(w + h v) - r0) / h + T v, h = the MATMFFD_DS step, formed and consumed on the device: no host synchronisation
static int ank_mult_enqueue(const double* d_v, double* d_y)
{
    const AnkKind& K = ank_last();
    const bool turb = g_ank.last == 1;
    const long n = K.ncell * K.nState;
    const int nS = K.nState;
    double* hdev = ank_scal(ANK_H);
    launch_ank_step(K.w0, d_v, n, 1.490116119384766e-08, 1e-6, g_ank.red + ANK_RED_SUMS, hdev, g_stream);
    if (ank_set_w_enqueue(K.w0, nS, true, d_v, hdev, turb)) return 1;
    if (ank_res_enqueue(K.flags)) return 1;
    LevelTab t;
    if (level_tab(1, &t)) return 1;
    if (turb)
        launch_ank_quotient_turb(t.tab, t.n, t.nx, t.ny, t.nz, d_v, K.r0, K.tsm, K.turbDiag, g_opts.turbResScale, hdev, d_y, g_stream);
    else
        launch_ank_quotient(t.tab, t.n, t.nx, t.ny, t.nz, nS, d_v, K.r0, K.tsm, K.tCells, K.turbDiag, g_opts.turbResScale, hdev, d_y, g_stream);
    return 0;
}

int adflow_gpu_ank_mult_dev(const double* d_v, double* d_y, long n)
{
    if (ank_mult_check("ank_mult", d_v, d_y, n)) return 1;
    if (ank_mult_enqueue(d_v, d_y)) return 1;
    return sync_and_check();
}

int adflow_gpu_ank_mult(const double* v, double* y, long n)
{
    if (ank_mult_check("ank_mult", v, y, n)) return 1;
    bool zero = true;                  // v = 0: y = 0 and no residual is evaluated
    for (long i = 0; i < n && zero; ++i) zero = v[i] == 0.0;
    if (zero) {
        memset(y, 0, sizeof(double) * n);
        HIPCHK(hipMemsetAsync(ank_scal(ANK_H), 0, ANK_NSCAL * sizeof(double), g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        return 0;
    }
    Stage s;
    return stage_open(&s, n, 2) || s.in(0, v) || ank_mult_enqueue(s[0], s[1]) || s.out(y, 1) || s.done();
}

// the kind whose base adflow_gpu_ank_mult / _solve / _last_h act on: the one set last, or the one selected here
int adflow_gpu_ank_select_base(unsigned flags)
{
    if (need_ready()) return 1;
    if (flags & ~ADFLOW_ANK_TURB) return fail("ank_select_base: flags = %u; accepted is ADFLOW_ANK_TURB", flags);
    if (!ank_kind(flags).haveBase)
        return fail("ank_select_base: no base state%s (call adflow_gpu_ank_set_base first)", ank_is_turb(flags) ? " of the turbulence KSP" : "");
    g_ank.last = ank_is_turb(flags) ? 1 : 0;
    return 0;
}

int adflow_gpu_ank_last_h(double* h)
{
    if (need_ready()) return 1;
    if (!ank_last().haveBase || !h) return fail("ank_last_h: no base state (call adflow_gpu_ank_set_base first)");
    HIPCHK(hipMemcpyAsync(h, ank_scal(ANK_H), sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

static int ank_gm_check(int level, const double* b, const double* x, long n, int restart, int maxIts, double rtol, double atol)
{
    if (gm_check_ranks("ank_solve", "adflow_gpu_ank_mult_dev")) return 1;
    if (level != 1) return fail("ank_solve: level %d; the matrix-free operator acts on level 1", level);
    if (ank_mult_check("ank_solve", b, x, n)) return 1;
    if (pc_check("ank_solve", level, b, x, n, false)) return 1;
    if (pc_sel().nState != ank_last().nState || pc_sel().ncell != ank_last().ncell)
        return fail("ank_solve: the factor was set up for nState = %d, the base state has nState = %d", pc_sel().nState, ank_last().nState);
    return gm_check_caps("ank_solve", restart, maxIts, rtol, atol);
}

int adflow_gpu_ank_solve_dev(int level, const double* d_b, double* d_x, long n, int restart, int maxIts, double rtol, double atol, int* its,
                             double* rnorm0, double* rnorm)
{
    if (ank_gm_check(level, d_b, d_x, n, restart, maxIts, rtol, atol)) return 1;
    if (gm_solve("ank_solve", ank_mult_enqueue, 0, d_b, d_x, n, restart, maxIts, rtol, atol, 0, its, rnorm0, rnorm)) return 1;
    return sync_and_check();
}

int adflow_gpu_ank_solve(int level, const double* b, double* x, long n, int restart, int maxIts, double rtol, double atol, int* its,
                         double* rnorm0, double* rnorm)
{
    if (ank_gm_check(level, b, x, n, restart, maxIts, rtol, atol)) return 1;
    DevBuf buf;                        // b and x of this call, not g_vec_dev
    HIPCHK(hipMalloc(&buf.p, sizeof(double) * 2 * n));
    const Stage s{n, (double*)buf.p};
    return s.in(0, b) || gm_solve("ank_solve", ank_mult_enqueue, 0, s[0], s[1], n, restart, maxIts, rtol, atol, 0, its, rnorm0, rnorm) ||
           s.out(x, 1) || s.done();
}

static int ank_phys_check(const double* w, const double* dw, long n, unsigned flags, double stepFactor, double stepMin, const double* lambda,
                          long* cells, int* nS)
{
    if (need_ready()) return 1;
#ifndef ADFLOW_NO_RCCL
    if (g_nranks > 1)
        return fail("ank_physicality_check: %d ranks in the communicator; the minimum is not reduced across ranks (the mpi_allreduce of "
                    "physicalityCheckANK is the host's)", g_nranks);
#endif
    if (flags & ~ANK_KIND_FLAGS) return fail("ank_physicality_check: flags = %u; accepted are ADFLOW_ANK_COUPLED or ADFLOW_ANK_TURB", flags);
    if (ank_vec_check("ank_physicality_check", w, dw, n, flags, cells, nS)) return 1;
    if (!lambda) return fail("ank_physicality_check: lambda is NULL");
    if (w == dw) return fail("ank_physicality_check: state and update are the same vector");
    (void)stepFactor; (void)stepMin;
    return 0;
}

// nS = 1 (ADFLOW_ANK_TURB): physicalityCheckANKTurb, the signed-ratio rule on the single entry and no density / energy rule
static int ank_phys_enqueue(const double* d_w, double* d_dw, long cells, int nS, double physLSTol, double physLSTolTurb, double stepFactor,
                            double stepMin, double lambda0)
{
    if (ank_red()) return 1;
    launch_ank_phys(d_w, d_dw, cells, nS, nS >= 5 ? 1 : 0, nS > 5 ? 5 : nS == 1 ? 0 : -1, 1.e-25, physLSTol, physLSTolTurb, stepFactor * stepMin,
                    lambda0, g_ank.red + ANK_RED_MIN, ank_scal(ANK_LAMBDA), g_stream);
    return 0;
}

int adflow_gpu_ank_physicality_check_dev(const double* d_w, double* d_dw, long n, unsigned flags, double physLSTol, double physLSTolTurb,
                                         double stepFactor, double stepMin, double* lambda)
{
    long cells; int nS;
    if (ank_phys_check(d_w, d_dw, n, flags, stepFactor, stepMin, lambda, &cells, &nS)) return 1;
    if (ank_phys_enqueue(d_w, d_dw, cells, nS, physLSTol, physLSTolTurb, stepFactor, stepMin, *lambda)) return 1;
    HIPCHK(hipMemcpyAsync(lambda, ank_scal(ANK_LAMBDA), sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));      // lambda goes to the host: synchronous whatever adflow_gpu_set_async says
    HIPCHK(hipGetLastError());
    return 0;
}

int adflow_gpu_ank_physicality_check(const double* w, double* dw, long n, unsigned flags, double physLSTol, double physLSTolTurb,
                                     double stepFactor, double stepMin, double* lambda)
{
    long cells; int nS;
    Stage s;
    if (ank_phys_check(w, dw, n, flags, stepFactor, stepMin, lambda, &cells, &nS) || stage_open(&s, n, 2) || s.in(0, w) || s.in(1, dw) ||
        ank_phys_enqueue(s[0], s[1], cells, nS, physLSTol, physLSTolTurb, stepFactor, stepMin, *lambda))
        return 1;
    if (nS != 5 && s.out(dw, 1)) return 1;       // only a turbulence entry is ever clipped
    return s.scalars(lambda, ank_scal(ANK_LAMBDA), 1) || s.done();
}

// computeUnsteadyResANK / computeUnsteadyResANKTurb (:2614-2786): the state is the one adflow_gpu_ank_set_w left (w - omega dW);
// blocketteRes with its closures, then r = the residual vector of the kind - omega T dW and its norm in one pass (k_ank_unsteady)
static int ank_unsteady_check(const double* dW, const double* r, long n, unsigned flags, const double* norm, long* cells, int* nS)
{
    if (ank_vec_check("ank_unsteady_res", dW, r, n, flags, cells, nS)) return 1;
    if (dW == r) return fail("ank_unsteady_res: update and result are the same vector (not done in place)");
#ifndef ADFLOW_NO_RCCL
    if (g_nranks > 1 && norm)
        return fail("ank_unsteady_res: %d ranks in the communicator; the norm is not reduced across ranks (pass norm = NULL to the _dev "
                    "form and reduce on the host)", g_nranks);
#endif
    const AnkKind& K = ank_kind(flags);
    if (!K.haveT)
        return fail("ank_unsteady_res: no pseudo-time term%s (call adflow_gpu_ank_time_step first)", ank_is_turb(flags) ? " of the turbulence KSP" : "");
    if (K.tLevel != 1 || K.tNState != *nS || K.tCells != *cells)
        return fail("ank_unsteady_res: the pseudo-time term was formed for nState = %d on level %d, the vectors have nState = %d on level 1",
                    K.tNState, K.tLevel, *nS);
    return 0;
}

static int ank_unsteady_enqueue(const double* d_dW, double omega, double* d_r, int nS, unsigned flags, bool wantNorm)
{
    if (ank_red()) return 1;
    LevelTab t;
    if (level_tab(1, &t)) return 1;
    const long groups = ank_unsteady_groups(t.n, t.nx, t.ny, t.nz);
    if (g_ank.partCap < groups) {
        HIPCHK(hipStreamSynchronize(g_stream));
        if (g_ank.part) (void)hipFree(g_ank.part);
        g_ank.part = nullptr; g_ank.partCap = 0; g_ank.bytesPart = 0;
        HIPCHK(hipMalloc((void**)&g_ank.part, sizeof(double) * groups));
        g_ank.partCap = groups; g_ank.bytesPart = sizeof(double) * groups;
    }
    if (ank_res_enqueue(flags, true)) return 1;
    if (level_tab(1, &t)) return 1;
    const AnkKind& K = ank_kind(flags);
    launch_ank_unsteady(t.tab, t.n, t.nx, t.ny, t.nz, nS, ank_is_turb(flags) ? 1 : 0, d_dW, K.tsm, K.tCells, K.turbDiag, g_opts.turbResScale, omega,
                        d_r, g_ank.part, wantNorm ? ank_scal(ANK_NORM) : nullptr, g_stream);
    return 0;
}

int adflow_gpu_ank_unsteady_res_dev(const double* d_dW, double omega, double* d_r, long n, unsigned flags, double* norm)
{
    long cells; int nS;
    if (ank_unsteady_check(d_dW, d_r, n, flags, norm, &cells, &nS)) return 1;
    if (ank_unsteady_enqueue(d_dW, omega, d_r, nS, flags, norm != nullptr)) return 1;
    if (!norm) return sync_and_check();          // no reduction, nothing goes to the host: honours adflow_gpu_set_async
    HIPCHK(hipMemcpyAsync(norm, ank_scal(ANK_NORM), sizeof(double), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int adflow_gpu_ank_unsteady_res(const double* dW, double omega, double* r, long n, unsigned flags, double* norm)
{
    long cells; int nS;
    Stage s;
    if (ank_unsteady_check(dW, r, n, flags, norm, &cells, &nS) || stage_open(&s, n, 2) || s.in(0, dW) ||
        ank_unsteady_enqueue(s[0], omega, s[1], nS, flags, norm != nullptr) || s.out(r, 1))
        return 1;
    return (norm && s.scalars(norm, ank_scal(ANK_NORM), 1)) || s.done();
}

// turbAPI::turbSolveDDADI (src/turbulence/turbAPI.F90:4-95) for Spalart-Allmaras:
// nSubIterTurb x [ sa_block(.false.) on every block ; whalo2(nt1:nt2, no p, viscosities) ]
int adflow_gpu_sa_solve(int level)
{
    if (need_ready()) return 1;
    if (g_opts.equations != ADFLOW_RANS) return fail("adflow_gpu_sa_solve needs equations = RANS");
    const int nit = std::max(1, (int)g_opts.nSubIterTurb);
    for (int it = 0; it < nit; ++it) {
        KParams kp = make_kparams(level, 1.0, 0);
        // sa_block(.false.) of every block: bcTurbTreatment first, applyAllTurbBCThisBlock(.true.) last (sa.F90:40-84)
        int rc = for_level(level, [&](Block* b) {
            if (b->v.nw < 6) return fail("RANS/SA needs nw = 6 (block has %d)", b->v.nw);
            return 0;
        });
        if (rc) return rc;
        if (turb_bc_treatment_enqueue(level, kp)) return 1;
        LevelTab t;
        if (level_tab(level, &t)) return 1;
        const bool marchRes = (g_sa_march == 1 && level_at_rest(level));
        if (marchRes) {
            if (ensure_sa_tiles(level)) return 1;
            launch_sa_march(t.tab, g_sa_tiles[level].first, g_sa_tiles[level].second, kp, g_stream, true);
        }
        launch_sa_solve_level(t.tab, t.n, t.nx, t.ny, t.nz, kp, g_stream, marchRes);
        if (turb_bc_apply_enqueue(level, kp, 1)) return 1;
        if (g_turb_bc_callback) {
            HIPCHK(hipStreamSynchronize(g_stream));
            g_turb_bc_callback(level, 1);
        }
        if (g_comm.count(std::make_pair(level, 2)))
            if (halo_exchange_enqueue(level, 6, 6, 0, 1, 2)) return 1;
    }
    return sync_and_check();
}

int adflow_gpu_set_turb_bc_callback(adflow_bc_callback fn)
{
    ++g_state_gen;
    g_turb_bc_callback = fn;
    return 0;
}

int adflow_gpu_res_norms(int level, double* sums, int n)
{
    if (need_ready()) return 1;
    if (!sums || n < 1 || n > 6) return fail("res_norms: n must be 1..6");
    if (!g_norm_dev) HIPCHK(hipMalloc((void**)&g_norm_dev, sizeof(double) * 8));
    HIPCHK(hipMemsetAsync(g_norm_dev, 0, sizeof(double) * 8, g_stream));
    int rc = for_level(level, [&](Block* b) {
        if (n > b->v.nw) return fail("res_norms: n=%d exceeds nw=%d", n, b->v.nw);
        launch_res_norms(b->v, n, g_norm_dev, g_stream);
        return 0;
    });
    if (rc) return rc;
#ifndef ADFLOW_NO_RCCL
    if (g_nccl && g_nranks > 1) NCCLCHK(ncclAllReduce(g_norm_dev, g_norm_dev, n, ncclDouble, ncclSum, g_nccl, g_stream));
#endif
    HIPCHK(hipMemcpyAsync(sums, g_norm_dev, sizeof(double) * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

// --------------------------------------------------------- instrumentation
int adflow_gpu_event_record(int slot)
{
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    if (slot < 0 || slot >= 64) return fail("event slot %d out of range", slot);
    HIPCHK(hipEventRecord(g_events[slot], g_stream));
    return 0;
}

int adflow_gpu_event_elapsed_ms(int a, int b, double* ms)
{
    if (a < 0 || a >= 64 || b < 0 || b >= 64 || !ms) return fail("bad event arguments");
    HIPCHK(hipEventSynchronize(g_events[b]));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, g_events[a], g_events[b]));
    *ms = f;
    return 0;
}

int adflow_gpu_march_stats(int level, double* out, int n)
{
    if (need_ready()) return 1;
    if (!out || n < 4) return fail("march_stats: n = %d (>= 4)", n);
    for (int q = 0; q < n; ++q) out[q] = 0.0;
    if (ensure_gf_tiles(level) || ensure_sa_tiles(level) || ensure_tiles(level)) return 1;
    // Spalart-Allmaras march: one trip per produced plane, four wavefronts
    {
        const auto& tt = g_sa_tiles[level];
        std::vector<int4> h((size_t)tt.second);
        if (tt.second > 0) HIPCHK(hipMemcpy(h.data(), tt.first, sizeof(int4) * h.size(), hipMemcpyDeviceToHost));
        for (const int4& t : h)
            if (t.x >= 0) out[0] += 4.0 * (t.w - t.z + 1);
    }
    // fused gradient + viscous march: every chunk marches its planes + 2 (k_visc_gf: mm = k0-1 .. k1+1), four wavefronts
    {
        const auto& tt = g_gf_tiles[level];
        std::vector<int4> h((size_t)tt.second);
        if (tt.second > 0) HIPCHK(hipMemcpy(h.data(), tt.first, sizeof(int4) * h.size(), hipMemcpyDeviceToHost));
        for (const int4& t : h)
            if (t.x >= 0) out[1] += 4.0 * (t.w - t.z + 3);
    }
    for (auto& kv : g_blocks) {
        if (std::get<0>(kv.first) != level || std::get<1>(kv.first) != 1) continue;
        const BlkView& v = kv.second->v;
        // tile table (k_roe_march, k_visc_march, ...): 60 columns x march_by rows x march_kch planes, kch + 1 trips per chunk
        int ntx, nty, ntz;
        euler_march_tiles(v, &ntx, &nty, &ntz);
        out[2] += 4.0 * ntx * nty * (v.nz + ntz);
    }
    return 0;
}

int adflow_gpu_sync(void)
{
    if (g_device < 0) return fail("adflow_gpu_init has not been called");
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g_stream));
    return 0;
}

int adflow_gpu_set_tuning(const char* key, int value)
{
    ++g_state_gen;
    if (!key) return fail("null tuning key");
    if (!strcmp(key, "euler_march")) { g_use_march = (value != 0); return 0; }
    if (!strcmp(key, "viscous_tiled")) { g_viscous_tiled = value; return 0; }
    if (!strcmp(key, "inviscid_march")) { g_inviscid_march = value; return 0; }
    if (!strcmp(key, "roe_march")) { g_roe_march = value; return 0; }
    if (!strcmp(key, "sa_march")) { g_sa_march = value; return 0; }
    if (!strcmp(key, "overlap")) { g_overlap = value; return 0; }
    if (!strcmp(key, "max_grid_z")) { g_max_grid_z = (value > 0) ? value : 65535; return 0; }
    if (!strcmp(key, "metric_from_x")) { g_metric_from_x = value; return 0; }
    if (!strcmp(key, "xcd_tiles")) {
        g_xcd_tiles = value;
        if (g_stream) (void)hipStreamSynchronize(g_stream);
        mg_graph_drop();       // a captured cycle holds the device pointer of the tile table (g_state_gen above retires it as well)
        for (auto& kv : g_tiles) (void)hipFree(kv.second.first);
        g_tiles.clear();
        return 0;
    }
    if (!strcmp(key, "phase_events")) {
        if (value != 0 && (value < 8 || value > 56)) return fail("phase_events: first slot must be 8..56 (or 0 = off)");
        g_phase_base = value;
        return 0;
    }
    if (!strcmp(key, "march_kch")) {
        if (value < 4) return fail("march_kch must be >= 4");
        g_march_kch = value;
        if (g_stream) (void)hipStreamSynchronize(g_stream);
        mg_graph_drop();
        for (auto* mp : {&g_tiles, &g_gf_tiles, &g_gf_tiles_int, &g_gf_tiles_bnd, &g_sa_tiles, &g_sa_tiles_int, &g_sa_tiles_bnd}) {
            for (auto& kv : *mp) (void)hipFree(kv.second.first);
            mp->clear();
        }
        return 0;
    }
    if (!strcmp(key, "split_eval")) { g_split_eval = value; return 0; }
    if (!strcmp(key, "test_fault")) { g_test_fault = value; g_mgg.failed = false; mg_graph_drop(); return 0; }
    if (!strcmp(key, "ad_cache")) { g_ad_cache = value; if (!value) { if (g_stream) (void)hipStreamSynchronize(g_stream); ad_drop(); } return 0; }
    if (!strcmp(key, "rvec_joint")) { g_rvec_joint = value; return 0; }
    if (!strcmp(key, "jac_snap")) { g_jac_snap = value; return 0; }
    if (!strcmp(key, "pc_fused")) { g_pc_fused = value; mg_graph_drop(); return 0; }
    if (!strcmp(key, "mg_graph")) { g_mg_graph = value; g_mgg.failed = false; mg_graph_drop(); return 0; }
    if (!strcmp(key, "comm_self")) {
        if (g_stream) (void)hipStreamSynchronize(g_stream);
        g_comm_self = value;
        for (auto& kv : g_comm) drop_comm_lists(kv.second);        // rebuilt at the next exchange
        return 0;
    }
    if (!strcmp(key, "dadi_pcr")) { g_dadi_pcr = value; mg_graph_drop(); return 0; }
    if (!strcmp(key, "ra_pcr")) { g_ra_pcr = value; mg_graph_drop(); return 0; }
    if (!strcmp(key, "dadi_upd")) { g_dadi_upd = value; mg_graph_drop(); return 0; }
    if (!strcmp(key, "gf_cus")) {
        // tests: the round size on a device with `value` CUs (0 = ask the device; -1 = chunks of march_kch planes, no fitting)
        g_gf_nofit = (value < 0);
        g_num_cus = value > 0 ? value : 0;
        if (g_stream) (void)hipStreamSynchronize(g_stream);
        mg_graph_drop();
        for (auto* mp : {&g_tiles, &g_gf_tiles, &g_gf_tiles_int, &g_gf_tiles_bnd, &g_sa_tiles, &g_sa_tiles_int, &g_sa_tiles_bnd}) {
            for (auto& kv : *mp) (void)hipFree(kv.second.first);
            mp->clear();
        }
        return 0;
    }
    return fail("unknown tuning key '%s'", key);
}

int adflow_gpu_set_async(int on)
{
    g_async = (on != 0);
    return 0;
}

int adflow_gpu_abi_sizes(int* opts_bytes, int* desc_bytes)
{
    if (opts_bytes) *opts_bytes = (int)sizeof(adflow_opts);
    if (desc_bytes) *desc_bytes = (int)sizeof(adflow_block_desc);
    return 0;
}

int adflow_gpu_abi_sizes2(int* bc_subface_bytes, int* comm_pattern_bytes)
{
    if (bc_subface_bytes) *bc_subface_bytes = (int)sizeof(adflow_bc_subface);
    if (comm_pattern_bytes) *comm_pattern_bytes = (int)sizeof(adflow_comm_pattern);
    return 0;
}

}  // extern "C"

// device buffers that outlive the blocks (vector staging, norm sums, surface nodes): released by adflow_gpu_finalize
static void free_side_buffers(void)
{
    free_xsurf();
    if (g_vec_dev) (void)hipFree(g_vec_dev);
    g_vec_dev = nullptr;
    g_vec_elems = 0;
    if (g_norm_dev) (void)hipFree(g_norm_dev);
    g_norm_dev = nullptr;
    if (g_floor_flag_dev) (void)hipFree(g_floor_flag_dev);
    g_floor_flag_dev = nullptr;
    if (g_snapreq.dev) (void)hipFree(g_snapreq.dev);
    g_snapreq = SnapReq();
#ifndef ADFLOW_NO_RCCL
    if (g_nccl) (void)ncclCommDestroy(g_nccl);
    g_nccl = nullptr;
    g_rank = 0;
    g_nranks = 1;
#endif
}
