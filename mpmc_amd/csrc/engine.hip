// engine.hip -- host side of the MI355X energy engine: persistent device context, kernel
// orchestration for one energy() evaluation, and the extern "C" ABI of include/mpmc_hip.h.
//
// Control flow of mpmc_hip_energy() mirrors reference src/energy/energy.c:67-226:
//   [polar]  rank metric -> dipole-tensor data (pair coefficients, or the expanded A matrix for the
//            Gauss-Seidel modes) -> static field -> SCF sweeps -> (Palmo) -> U_pol      main stream
//   [lj]     fused pair kernel (LJ + FH) + cached long-range correction                  side stream
//   [es]     real-space part in the same pair kernel, reciprocal kernel, self term       side stream
// Everything pairwise is resident and updated incrementally after a move (coefficients, tile partial
// sums of the pair / field / LRC kernels); the only host<->device traffic per call is the moved
// molecule's coordinates in (kernel arguments) and a 16-double result record out (mapped host memory; in the
// Jacobi-type modes in two parts, one per stream, so that a steady-state step has no cross-stream event at all: the
// side stream takes the move from its own kernel arguments and publishes its own slots).
// The reference plugin re-allocated and re-uploaded everything per call (polar_cuda_pcg.cu:221-401).
#include "../../include/mpmc_hip.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <tuple>
#include <utility>
#include <ctime>
#include <numeric>
#include <atomic>
#include <string>
#include <vector>

#include "device_common.h"
#include "step_plan.h"
#include "kernels_pair.h"
#include "kernels_disp.h"
#include "kernels_rdforms.h"
#include "kernels_at.h"
#include "kernels_crystal.h"
#include "kernels_vdw.h"
#include "kernels_polar.h"
#include "kernels_exact.h"
#include "kernels_gs.h"
#include "kernels_gs_chain.h"
#include "kernels_resident.h"
#include "kernels_symv.h"
#include "kernels_coef.h"
#include "kernels_volume.h"
#include "kernels_cavity.h"
#include "kernels_dimer.h"
#include "kernels_trial.h"

using namespace mpmc;

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
// contexts alive per device in this process: the resident solver needs the device to itself (kernels_resident.h)
static std::atomic<int> g_ctx_on_device[64];

static int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail("MPMC_HIP: %s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                 \
    } while (0)

extern "C" const char *mpmc_hip_last_error(void) { return g_err.c_str(); }
extern "C" int mpmc_hip_abi_version(void) { return MPMC_HIP_ABI_VERSION; }
extern "C" int mpmc_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
// Owners of the context's device memory, pinned host memory, streams and events: move-only, released by their
// destructors.  They convert to the raw pointer / handle, so that kernel arguments and HIP calls take them as they are.
template <typename T, bool kPinned>
class HipBuffer {
  public:
    HipBuffer() = default;
    HipBuffer(HipBuffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    ~HipBuffer() { reset(); }
    // frees the current block, then allocates `count` elements (host_flags: hipHostMalloc's); empty on failure
    hipError_t alloc(size_t count, unsigned host_flags = hipHostMallocDefault) {
        reset();
        void *p = nullptr;
        hipError_t e;
        if constexpr (kPinned)
            e = hipHostMalloc(&p, count * sizeof(T), host_flags);
        else
            e = hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess) p_ = static_cast<T *>(p), n_ = count;
        return e;
    }
    void reset() {
        if (p_) {
            if constexpr (kPinned)
                hipHostFree(p_);
            else
                hipFree(p_);
        }
        p_ = nullptr;
        n_ = 0;
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }  // elements
    operator T *() const { return p_; }

  private:
    T *p_ = nullptr;
    size_t n_ = 0;
};
template <typename T>
using DevBuf = HipBuffer<T, false>;
template <typename T>
using PinnedBuf = HipBuffer<T, true>;

template <typename H, hipError_t (*kDestroy)(H)>
class HipHandle {
  public:
    HipHandle() = default;
    HipHandle(HipHandle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~HipHandle() { reset(); }
    // releases the current handle; returns where a create call writes the new one
    H *out() {
        reset();
        return &h_;
    }
    operator H() const { return h_; }

  private:
    void reset() {
        if (h_) kDestroy(h_);
        h_ = nullptr;
    }
    H h_ = nullptr;
};
using HipStream = HipHandle<hipStream_t, hipStreamDestroy>;
using HipEvent = HipHandle<hipEvent_t, hipEventDestroy>;

constexpr int kMaxDirty = 64;  // more moved atoms than this => full A rebuild (= DirtyList capacity)

enum TimeClass { T_PAIR = 0, T_RECIP, T_FIELD, T_AMAT, T_SWEEP, T_PALMO, T_OTHER, T_EVPAIR, T_NCLASS };

struct TimeRec {
    int cls;
    hipEvent_t a, b;
};

enum ResSlot {
    R_RD_PAIR = 0,  // 4 pair channels: rd, es_real, es_intra, spare
    R_ES_REAL = 1,
    R_ES_INTRA = 2,
    R_LRC = 4,
    R_RECIP = 5,
    R_SELF = 6,
    R_UPOL = 7,
    R_RRMS = 8,
    R_GS_ERR = 9,  // bit 0 / 1: the persistent Gauss-Seidel kernel of view 0 / 1 gave up on a hand-off
    R_RMIN = 10,
    R_RANKCHG = 11,  // speculative ranked call: 1 = the ranking metric differs from the one the ranked view was built for
    R_DISP = 12,      // disp_expansion: the dense pair sum (kernels_disp.h) ...
    R_DISP_LRC = 13,  // ... and its long-range correction; both read as zero outside that mode
    R_AT = 14,        // axilrod_teller: the triple-dipole sum (kernels_at.h); reads as zero outside that mode
    R_RDC_SELF = 15,  // rd_crystal: the self part (kernels_crystal.h); its pair part and long-range correction take R_DISP and
                      // R_DISP_LRC, which the two modes cannot both want (energy() refuses the combination)
    R_COUNT = 16,
    // polarvdw (kernels_vdw.h) adds no slot: the repulsion-only sum and its long-range correction take R_DISP and R_DISP_LRC,
    // the eigenvalue sum e_total takes R_AT and lr_corr takes R_RDC_SELF -- energy() refuses the mode together with each of
    // the three modes that own them.  The close-contact count rides in the spare fourth pair channel.
    R_VDW = R_AT,
    R_VDW_LRC = R_RDC_SELF,
    R_CONTACTS = 3
};

// A "sweep view" = the polarizable atoms, compacted, in the order the SCF sweep visits them.
// View 0: atom order (Jacobi, polar_gs and the first polar_gs_ranked sweep); view 1: ranked order.
// Non-polarizable sites have mu = 0 and their rows are skipped by the reference
// (thole_iterative.c:34-39), so neither their rows nor their columns of A are ever needed by the
// solver: the device matrix is (3 nv)^2 instead of (3 N)^2.
struct SweepView {
    int nv = 0, nvpad = 0, cap = 0;
    DevBuf<int> d_idx;  // atom index of view slot k
    DevBuf<double> px, py, pz, palpha;
    DevBuf<int> pflags;
    DevBuf<double> A;
    bool A_valid = false;  // A matches the configuration as of the last energy() (minus `dirty` atoms)
    DevBuf<double2> C;  // pair-coefficient tiles {c3, c5} (kernels_coef.h), the default sweep storage
    int ntld = 0;          // tile stride of C: the number of 64-atom tiles the view can grow to
    DevBuf<double> energy_part;  // [cap/64][2] per-block sums for U_pol and <rrms>
    bool C_valid = false;
    bool pos_valid = false;  // px/py/pz/palpha/pflags match the configuration (moves are applied to both copies)
    unsigned long long ranked_call = 0;  // view 1: the energy() call that last walked (and so maintained) it
    DevBuf<int> d_slot;  // device copy of slot_of_atom (padded with -1)
    std::vector<int> slot_of_atom;  // atom index -> view slot, -1 if not in the view
    DevBuf<double> mupub;  // Gauss-Seidel chain: the published dipoles of a sweep, planar per block (hand-off buffer)
    DevBuf<double> es, mu0, mu1, munew, y, efind, efchg, rrms;
    DevBuf<double> tmu0;  // a Jacobi sweep's sums T mu, kept for the energy of a solve whose last sweep is deferred (odd counts)
    DevBuf<unsigned> gsflags;  // [8] gs_chain_kernel: ticket counter, sticky error word, breadcrumbs
    // Gauss-Seidel chain (kernels_gs_chain.h): cached inverses of the diagonal blocks and expanded sub-diagonal tiles
    DevBuf<double> Minv;         // [cap/64][kMinvDoubles]
    DevBuf<double> Lnb[kGsMaxLag];  // [k-1]: [cap/64][kPnbDoubles], L(k)_t = M_t D T(t,t-k)
    int Lnb_lags = 0;            // how many of them are allocated
    int nlag = 0, nlag_built = 0;   // lags this view's chain uses / has matrices for (decided at a whole-view rebuild)
    long long last_full_call = -1;  // energy_calls of the view's last whole rebuild
    int full_streak = 0;            // consecutive calls that rebuilt it as a whole
    unsigned long long C_epoch = 0;   // bumped by every full build of C
    unsigned long long M_epoch = 0;   // C_epoch the chain data were last fully built under (0: never)
    unsigned long long M_call = 0;    // energy() call that last maintained them
    int rebuild_from = -1;            // >= 0: the view's order changed from this 64-atom block on (set_sweep_order):
                                      // blocks in front of it keep their data, the rest is rebuilt at the next energy()
    DevBuf<double> Srow;  // partial sums of the symmetric sweep
    double *Zcol = nullptr;  // (inside Srow)
    // resident Jacobi solver (kernels_resident.h): partial-sum slots (sentinel between calls), published dipoles
    DevBuf<double> resP;
    int res_pld = 0;
    bool resP_armed = false;
    DevBuf<double> respub;
    std::vector<int> h_idx;
};

// The sweeps of a fixed-count plain Jacobi solve that are not launched yet (run_polarization(), defer_last_sweep()): U_pol
// does not need them, whoever asks for mu / E_ind does (complete_pending_sweep()).  Sweep n always; sweeps m + 1 .. n - 1
// (m = ceil(n / 2)) as well when the call's record went out behind the finish of sweep m, in launch order.  Every entry
// carries the buffers of the mu0 / mu1 ping-pong the call would have given it and its own parameters; view and box are the
// call's.  Everything the launches take that is not device state travels here; the device state they read (view
// coordinates, coefficients, E_static, mu_m) and the buffers they write (the other mu buffer, E_ind, the sweep scratch) stay
// as the call left them until something listed in DESIGN.md section 3 changes them -- which completes the sweeps first --
// or the next energy_begin() drops them.  Copyable: the step graph saves and restores it.
struct PendingSweep {
    struct One {
        const double *mu_in = nullptr;
        double *mu_out = nullptr;
        SweepParams sp;
    };
    std::vector<One> sweeps;  // in launch order; empty: nothing pending
    struct SweepView *view = nullptr;
    DevBox bx;
    void drop() { sweeps.clear(); }
};

// The kernels of one steady-state MC step whose arguments change from step to step; every other node of
// the captured graph is replayed as it was.
enum GraphSlotId { GS_MOVES = 0, GS_COEF, GS_FIELD, GS_PAIR, GS_RECIP, GS_PUBLISH, GS_NSLOT };
enum GraphMode { GM_DIRECT = 0, GM_CAPTURE = 1, GM_UPDATE = 2 };
struct StepGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    void *func[GS_NSLOT] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipGraphNode_t node[GS_NSLOT] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool valid = false;
    unsigned long long rev = 0;  // config_rev it was captured under
    // what the captured call left in the context besides device work
    int iterations = 0;
    struct SweepView *result_view = nullptr;
    const double *result_mu = nullptr;
    PendingSweep psweep;  // (never part of the capture: a replay leaves the same sweeps pending)
    const double *energy_part = nullptr;
    int energy_nt = 0;
    int recip_chunks = 0, pair_rows_to_sum = 0;
    unsigned res_zero_mask = 0;
};

// The knobs of mpmc_hip_set_option(), with their defaults: one member per row of kOptions (below), which names them.
struct EngineOptions {
    int pair_coef = 1;          // Jacobi/Palmo sweeps on pair coefficients (0: on the expanded A matrix)
    int incremental = 1;        // "incremental_amatrix"
    int incremental_pairs = 1;  // LJ/Ewald-real and static-field tile partials persist between calls
    int overlap = 1;            // "overlap_streams"
    int side_after = 1;         // feed the LJ/Ewald stream after this many sweeps are enqueued
    int symmetric = 1;          // "symmetric_sweep"
    int sym_mode = 0;           // bit 0: alternate sweep direction, bit 1: default-policy loads
    int timing = 1;             // 0: no events, 1: sweep kernels + total only, 2: every kernel class
    int timing_interval = 32;   // timing 1 / -1: every how many calls
    int persistent_gs = 1;
    int spec_rank = 1;          // "speculative_ranking": 0 = polar_gs_ranked asks the host for the sweep order in every call (A/B)
    int fuse_tensor = 1;        // (round 2's A/B switch; accepted and ignored: the chain no longer uses tensor tiles)
    int gs_lags = 3;            // cached neighbour matrices of the chain, 2 .. kGsMaxLag (kernels_gs_chain.h)
    int gs_build_fork = 1;      // 0 = the builder in the main stream (A/B)
    int gs_side_waves = 0;      // 16 = the OTHER view's rebuild in the side stream always with 16-wave workgroups;
                                // 0 = the fastest geometry that leaves the chain kernel its CUs
    int rank_view_side = 1;     // a host-sorted ranked view is (re)built on the side stream (0: main stream, behind the first sweep)
    int gs_fold_upper = 1;      // the chain's workgroups add up pair_upper_kernel's row sums themselves
    int gs_fold_finish = 1;     // gs_chain_kernel's workgroups do gs_finish_kernel's work for their block
    int rank_late = 1;          // polar_gs_ranked's side-stream ranking work is enqueued behind the first sweep
    int resident = 1;           // "resident_jacobi": fixed-count Jacobi-type solves as one launch, tiles in registers
    int res_fold = 16;          // "resident_fold": views of up to this many blocks run the solve without finisher
                                // workgroups (jacobi_folded_kernel); 0 = always with finishers
    int res_side = 0;           // "resident_side": 1 = feed the LJ/Ewald stream BEFORE the resident launch
    int sweep_alternate = 1;    // pair_sweep_kernel walks each XCD's tiles forwards / backwards in turn
    int sweep_nt = -1;          // non-temporal coefficient loads in pair_sweep_kernel: 1 always, 0 never,
                                // -1 = only when the tile set cannot stay in the 256-MB Infinity Cache
    int sweep_split = -1;       // half-tile workgroups in pair_sweep_kernel: 1 always, 0 never, -1 by size
    int fuse_moves = 1;         // the step's move is applied inside view 0's coefficient update
    int gs_fuse_moves = 1;      // Gauss-Seidel modes: the move rides in the coefficient update of view 0
    int fuse_field = 1;         // the move + coefficient update ride inside the field kernel's launch
    int fuse_recip = 1;         // the reciprocal-space partials ride in the pair kernel's launch
    int split_record = 1;       // the side stream publishes its own part of the result record
    int side_moves = 1;         // 0 = fork event after the main stream's move (A/B; same bits)
    int res_stamps = 0;         // "resident_stamps", diagnostic: the next resident launches print their hand-off time line
    int sweep_ablate = 0;       // timing-only ablations of pair_sweep_kernel (wrong results)
    int res_fault = 0;          // "resident_fault", test hook: the next resident launch loses a hand-off (-> fallback)
    int gs_stamps = 0;          // diagnostic: the next Gauss-Seidel sweeps print where a block's time goes (slow)
    int inv_stamps = 0;         // diagnostic: time stamps inside gs_block_inverse_kernel (main stream launches)
    int gs_ablate = 0;          // timing-only ablations of the chain kernel (wrong results; tools/gs_ablate.py)
    int gs_fault_sweep = 0;     // test hook: in Gauss-Seidel sweep number `value` (1-based) block 1 never publishes
    int graph = 0;              // "step_graph": off by default, see graph_step()
};

// What belongs to ONE evaluation: begin_call() resets it, enqueue_direct() / graph_step() fill it in, energy_end() reads what
// it needs after the wait.  Nothing here carries information from one call to the next.
struct CallState {
    // predicates of the call (enqueue_direct)
    bool do_polar = false;        // the polarization chain runs
    bool gs_mode = false;         // polar_gs or polar_gs_ranked
    bool exact = false;           // the exact dipoles (mpmc_hip_set_exact_polar): no sweep of any kind runs
    bool two_streams = false;     // the LJ / Ewald kernels run on the side stream beside it
    bool plain_launches = false;  // neither captured into a step graph nor eligible to be ("step_graph" off)
    DirtyBlocks dirty_blocks;             // 64-atom blocks of the atoms moved since the last call
    DirtyBlocks lrc_blocks;               // ... and of lrc_dirty_atoms (n = 0: none, or more than the list holds), which every
    bool lrc_edited = false;              //     long-range correction of the call consumes: lrc_edited = that list is not empty
    bool pair_part_valid_before = false;  // pair_part_valid when the call started (after collect_dirty_blocks)
    bool moves_deferred = false;  // pending moves not yet applied: they ride in view 0's coefficient update ...
    bool moves_in_pair = false;   // ... or inside the pair kernel's launch (steps without polarization)
    bool side_carry = false;      // ... and the side stream's pair kernel carries the same move itself (side_moves):
    MoveList side_moves;          //     no fork event between the two streams in a steady-state polarizable step
    MoveList pair_moves;          // the move the pair kernel's launch carried: the dense tile kernels behind it take it too
    MoveList side_apply;          // a move the main stream applied with apply_moves_kernel: the side stream applies it
    bool side_applied = false;    //     too (a launch of its own, in front of its first kernel) instead of waiting for an event
    bool coef_job_valid = false;  // setup_view() left the coefficient update of this step for launch_field()
    bool coef_job_fork = false;   //   ... which then also records the fork event behind it
    CoefJob coef_job;
    bool build_join_pending = false;  // the main stream has not yet waited for the builder launch of this call
    bool rank_on_side = false;        // ranking metric computed and copied to the host on the side stream
    int gs_sweeps = 0;                // Gauss-Seidel sweeps enqueued so far
    bool gs_used[2] = {false, false};  // the persistent kernel ran on view 0 / 1: its error word travels with the record
    bool polar_first = false;     // the chain is enqueued up to its first sweep before the side stream is fed (plan_call)
    bool side_open = false;       // run_polarization() may feed the side stream now (feed_side_stream; see enqueue_direct)
    bool side_done = false;       // enqueue_side_stream() has run in this call ...
    int side_rc = 0;              //   ... and returned this
    bool may_publish_early = false;  // this call may publish behind the finish of sweep m = ceil(n / 2), the finish that
    bool published = false;          //   completes U_pol (publish_early; see enqueue_direct); published: it did ...
    int publish_rc = 0;              //   ... and launch_publish() returned this
    bool recip_fused = false;     // the reciprocal-space partials rode in the pair kernel's launch
    int recip_chunks = 0;         // chunk sums the publish kernel folds (0: R_RECIP was written directly)
    int pair_rows_to_sum = 0;     // tile partials of the pair kernel the publish kernel has to add up
    unsigned res_zero_mask = 0;   // result slots the publish kernel writes as zero
    // what energy_end() needs to know about the call it collects
    bool split = false;           // the side stream published its own part of the record (two sequence numbers)
    bool resident = false;        // the resident kernel was used
    bool spec_rank = false;       // enqueued speculatively (polar_gs_ranked)
    bool timed = false;           // events were recorded
    int iterations = 0, iter_success = 0;
};

// A sum kept as per-tile partials and, added up in a fixed order, in a slot of d_res (kernels_tile.h).  valid: both are those
// of the current parameters, box and tile grid and of the configuration before the pending moves.
struct TileSum {
    DevBuf<double> part;
    bool valid = false;
};

struct mpmc_hip_ctx {
    // ---- configuration and box
    int device = 0;
    int num_cus = 256;
    int max_atoms = 0, max_npad = 0;
    int n = 0, npad = 0;
    EngineOptions opt;
    CallState call;
    mpmc_hip_params par;
    bool have_params = false, have_box = false, have_atoms = false;
    double basis[3][3], recip[3][3];
    double pbc_cutoff_in = 0.0, cutoff = 0.0, volume = 0.0, ewald_alpha = 0.0, polar_ewald_alpha = 0.0;
    bool box_ortho = false; // every off-diagonal basis entry is exactly zero
    double coord_max = 0.0; // max |coordinate| of everything sent since the last upload (guards the fp32 screen)
    unsigned long long config_rev = 1;   // bumped by everything that changes what an energy() call enqueues
    unsigned long long energy_calls = 0;
    bool in_flight = false;         // between energy_begin() and energy_end()
    // ---- streams and events (declared in front of the buffers used on them: destroyed after those)
    HipStream stream;
    HipStream stream2;              // pair / reciprocal kernels overlap the polarization chain
    HipStream stream3;              // the chain-data builder of the main stream's view runs here, beside that stream's next kernels
    HipEvent ev_fork, ev_join;
    HipEvent ev_rank;
    HipEvent ev_bfork, ev_bjoin;
    HipEvent ev_order;
    // SoA configuration (HBM)
    DevBuf<double> d_x, d_y, d_z, d_q, d_alpha, d_eps, d_sig, d_molmass;
    DevBuf<int> d_mol, d_flags;
    MoveList pending;               // coordinates handed over by update_atoms(), applied at the next energy()
    std::vector<int> dirty_atoms;   // atoms moved by update_atoms() since the last energy()
    bool all_dirty = true;
    bool staged_copies = false;          // coordinates reached the device outside the MoveList since the last call
    bool main_writes = false;            // the MAIN stream was given writes of coordinates / parameters / the slot map outside
                                         // the MoveList since the last call (staged copies, an upload, edits, a new sweep
                                         // order): the side stream must then wait for an event recorded behind them -- it may
                                         // not just apply the queued move for itself (side_apply / side_carry)
    // ---- sweep views and polarization results: full-size per-atom vectors (atom order) + the two sweep views
    SweepView view[2];
    DevBuf<double> d_es, d_mu, d_efind, d_efchg, d_tmp3;
    DevBuf<unsigned long long> d_errmax;
    bool have_polar_result = false;
    // where the last polarization result lives (view order); scattered to atom order on demand
    SweepView *result_view = nullptr;
    const double *result_mu = nullptr;
    bool results_scattered = true;
    PendingSweep psweep;            // the solve's sweeps that the last call left to the first reader of their output
    const double *energy_part = nullptr;  // per-block energy sums to fold in publish_result_kernel (or null)
    int energy_nt = 0;
    bool es_stale = false;  // d_es (atom order) not yet reduced from the field partials
    int es_slots = 0;
    int sweep_parity = 0;
    int gs_qoff = 0;                       // offset (doubles) of the q_t hand-off buffer inside a view's mupub
    DevBuf<unsigned long long> d_stamps, d_istamps;  // diagnostics: in-kernel time stamps (gs_stamps / resident_stamps, inv_stamps)
    // ---- pair / field / reciprocal caches
    DevBuf<double> d_pairpart;      // [ntile*ntile][4]
    bool pair_part_valid = false;   // d_pairpart holds the tile partials of the configuration before the pending moves
    DevBuf<double> d_fieldpart;     // [nchunk][3][npad]
    bool field_part_valid = false;  // same for d_fieldpart (real-space static field)
    int field_key = -1;             // mode / chunking the resident field partials were made with
    TileSum lrc;                    // [ntile*ntile] the (cached) long-range correction, R_LRC
    // ---- disp_expansion (PHAHST, mpmc_hip_set_dispersion): d_eps / d_sig then hold the exponent b and the range rho, the
    // LJ kernels are handed d_zero in their place (every LJ pair and the LJ long-range correction give exactly 0)
    bool disp_on = false;
    DispParams disp_par = {0, 0, 0};
    DevBuf<double> d_c6, d_c8, d_c10, d_zero;
    TileSum disp;                   // [ntile*ntile] the dense pair sum, R_DISP
    TileSum disp_lrc;               // [ntile*ntile] its long-range correction, R_DISP_LRC: parameters, cutoff and volume only
    // ---- axilrod_teller (mpmc_hip_set_axilrod_teller): the triple-dipole term, kernels_at.h
    bool at_on = false;
    DevBuf<double> d_at_a, d_at_g;  // per atom: alpha * 6.7483345 and 1 / (c9 / a^3)
    TileSum at;                     // [at_unit_count(ntile)][kAtSplit] block-triple partials, R_AT
    double three_body = 0.0;        // the term of the last completed energy_end() (0 outside the mode)
    // ---- rd_crystal (mpmc_hip_set_rd_crystal): Lennard-Jones over lattice images, kernels_crystal.h.  A context setting:
    // it carries no per-atom data and persists across uploads.  The LJ kernels are handed d_zero, as under disp_expansion.
    int rdc_order = 0;              // 0 = off, 1 .. kRdcMaxOrder
    TileSum rdc;                    // [ntile*ntile] the image sum, R_DISP
    TileSum rdc_static;             // [ntile*ntile] the long-range correction at cutoff_c, R_DISP_LRC; valid covers the self
                                    // part (R_RDC_SELF) too: both are those of the current parameters, box and rd_lrc
    int rdc_static_lrc = -1;        // the rd_lrc they were made under
    // ---- the other pair potentials (mpmc_hip_set_rd_form): Silvera-Goldman, DREIDING, buffered 14-7, and Lennard-Jones
    // under any mixing rule, kernels_rdforms.h.  A context setting like rd_crystal.  The LJ kernels are handed d_zero.
    int rd_form = 0;                // RdForm; 0 = the standard path
    int rd_mix = 0;                 // RdMix
    TileSum rdf;                    // [ntile*ntile] the dense pair sum, R_DISP
    TileSum rdf_lrc;                // [ntile*ntile] the LJ form's long-range correction, R_DISP_LRC
    bool negative_sigma = false;    // the upload holds a sigma < 0 (Waldman-Hagler leaves such a pair's epsilon unset)
    mpmc_hip_params par_user;       // what set_params() brought; `par` is that with rd_only forced on under the SG form
    // ---- polarvdw (mpmc_hip_set_vdw): coupled-dipole many-body van der Waals + repulsion-only Lennard-Jones, kernels_vdw.h.
    // The LJ kernels are handed d_zero, as under disp_expansion.
    bool vdw_on = false;
    DevBuf<double> d_vdw_w;         // per atom: omega (atomic units), zero for pad atoms
    DevBuf<int> d_vdw_idx;          // the sites of the matrix (k != 0), in atom order: atom slot ...
    DevBuf<double> d_vdw_k;         // ... and k = sqrt(alpha) * omega
    int vdw_na = 0;
    DevBuf<double> d_vdw_C;         // [3 na][3 na], destroyed by every solve
    DevBuf<double> d_vdw_vec;       // v, p, d, e, lambda: 3 na doubles each; then tau and the e_iso scratch slot
    TileSum vdw;                    // (no partials) valid: d_res[R_VDW] is e_total of the configuration before the pending moves
    TileSum vdw_lrc;                // [ntile*ntile] lr_corr, R_VDW_LRC
    TileSum rep;                    // [ntile*ntile] the repulsion-only pair sum, R_DISP
    TileSum rep_lrc;                // [ntile*ntile] its long-range correction, R_DISP_LRC
    struct VdwMolecule {
        int type, first_site, sites;  // type id; its run of sites in d_vdw_idx
    };
    std::vector<VdwMolecule> vdw_mols;   // the molecules of the upload, in upload order
    std::map<int, double> vdw_iso;       // e_iso per type id, from the first molecule of the type seen (vdw.c:262-320); kept
                                         // across uploads while the mode stays on
    double vdw_e_iso = 0.0;              // its sum over the molecules, in upload order
    bool vdw_iso_summed = false;
    double vdw_energy = 0.0;             // the term of the last completed energy_end() (0 outside the mode)
    double vdw_terms[5] = {0, 0, 0, 0, 0};  // ... and e_total, e_iso, lr_corr, the repulsion sum, its long-range correction
    // ---- exact dipoles (mpmc_hip_set_exact_polar): blocked Cholesky of view 0's matrix, kernels_exact.h.  A context setting:
    // it persists across uploads.  Nothing below is allocated while the mode is off.
    bool exact_polar = false;
    // ---- the dipole tensor (mpmc_hip_set_thole_model): a context setting, persists across uploads
    int thole_damp_type = 2;        // the reference's values: 0 off, 1 linear, 2 exponential
    bool thole_wolf_full = false;   // polar_wolf_full (exponential only)
    DevBuf<double> d_chol_W;        // [3 nvpad][3 nvpad] the work copy, L in its lower triangle after a call
    DevBuf<double> d_chol_vec;      // b, y, x of the substitutions: [3][3][3 nvpad]
    DevBuf<unsigned> d_chol_flag;   // [0]: a pivot of this call's factorization was not positive
    DevBuf<double> d_chol_tensor;   // [9]
    int chol_nv = 0, chol_nvpad = 0;  // the view the factor in d_chol_W is of (chol_nv = 0: none)
    bool chol_done = false;         // ... and an energy_end() has collected that call
    bool chol_failed = false;       // ... whose flag word was set
    // ---- cavity_autoreject_absolute (mpmc_hip_set_autoreject): a context setting, persists across uploads
    double autoreject_scale = 0.0;       // 0 = off
    long long close_contacts = 0;        // of the last completed energy_end()
    // ---- cavity_bias (mpmc_hip_set_cavity_grid): the cavity grid, kernels_cavity.h.  A context setting: it persists across
    // uploads and is independent of the atom slots -- the caller names the positions that are binned, leave and enter.
    int cav_G = 0, cav_P = 0;            // cavity_grid_size (0 = off) and G^3
    double cav_radius = 0.0, cav_T = 0.0;  // cavity_radius; the smallest double with sqrt(T) >= radius
    DevBuf<double> d_cav_pos;            // [3][P] grid point positions ...
    bool cav_pos_valid = false;          // ... of the current box
    DevBuf<int> d_cav_occ;               // [P]
    bool cav_occ_valid = false;          // binned since the grid was set / the box changed
    DevBuf<int> d_cav_open;              // [P] open_list of the last update
    int cav_open = -1;                   // its length (-1: no update since the occupancy was last replaced)
    int cav_incremental = 1;             // option "cavity_incremental": 0 = cavity_update answers 1 to every non-empty edit
    DevBuf<int> d_cav_blk;               // [2][ceil(P / 256)] open points per workgroup, and their exclusive scan
    DevBuf<int> d_cav_cnt;               // [CAV_NCOUNTER]
    DevBuf<double> d_cav_atoms, d_cav_darts;  // [3][n] positions of a full bin; [n_darts][3]
    DevBuf<int> d_cav_dart_hit;          // [n_darts] 1 = the dart lies in an open sphere
    PinnedBuf<double> h_cav_stage;       // pinned staging of either (each call that fills it waits for its copy)
    PinnedBuf<double> h_cav;             // pinned, mapped: the CavRecord
    double *h_cav_dev = nullptr;
    unsigned long long cav_seq = 0;
    // ---- dimer scans (mpmc_hip_dimer_energies / _grid_means, engine_dimer.inc): buffers of their own, grown on demand;
    // they share nothing with the resident configuration
    DevBuf<unsigned char> d_dimer_mols;  // one DimerMols
    DevBuf<double> d_dimer_rot[2];       // [K][9] rotation matrices per molecule
    DevBuf<double> d_dimer_r;            // [nconf] separations (list form)
    DevBuf<double> d_dimer_tab[2];       // [K][16][3] rotated sites per molecule
    DevBuf<double> d_dimer_out;          // list form: es, rd, polar [3][nconf]; grid form: chunk sums [3][nchunk]
    DevBuf<int> d_dimer_status;          // list form [nconf]; grid form [nchunk] non-converged placements
    DevBuf<double> d_dimer_mu;           // list form, on request [nconf][32][3]
    DevBuf<double> d_dimer_means;        // [3] + the non-converged count
    // ---- trial placements (mpmc_hip_trial_energies, engine_trial.inc): what the last completed energy() returned and
    // under which config_rev, and buffers of the batched path's own, grown on demand
    bool result_valid = false;           // an energy_end() has completed since the last energy_begin()
    unsigned long long result_rev = 0;   // config_rev at that moment
    mpmc_hip_result last_result;
    unsigned long long trial_calls = 0;  // calls that passed their checks
    int trial_batched = 1;               // option "trial_batched": 0 = the serial path in every mode (A/B; the batched path's check)
    DevBuf<double> d_trial_xyz;          // [ntrial][count][3]
    DevBuf<double> d_trial_pair;         // [ntrial + 1][2] rd, es_real of the molecule; row 0 = the current placement
    DevBuf<double> d_trial_chunk;        // [ntrial + 1][ceil(nk / 64)]
    DevBuf<double2> d_trial_srest;       // [nk] the structure factor without the molecule
    DevBuf<double> d_trial_out;          // [ntrial] energies, then [ntrial][3] terms
    double lrc_cached = 0.0;
    DevBuf<KVec> d_kvec;
    int nk = 0;
    bool kvec_valid = false;
    int kvec_kmax = -1;
    DevBuf<double2> d_sfpart;       // [block][nk] partial structure factors of the reciprocal-space sum
    bool recip_part_valid = false;
    DevBuf<double> d_recipsum;      // [ceil(nk/64)] per-chunk sums of w_k |S(k)|^2, folded by the publish kernel
    bool self_valid = false;        // d_res[R_SELF] holds the Ewald self term of the current charges
    double self_alpha = 0.0;
    DevBuf<KVecF> d_kvecf;          // k list weighted with polar_ewald_alpha (Ewald static field)
    DevBuf<double2> d_sf;
    int nkf = 0;
    double kvecf_alpha = -1.0;
    int kvecf_kmax = -1;
    bool kvecf_valid = false;
    // ---- ranking
    DevBuf<double> d_rank;
    DevBuf<double> d_rankpart;      // scratch of the ranking metric (per-tile minima)
    // polar_gs_ranked without a host round trip: the ranked view (1) is kept for the walk of the previous call and
    // the whole evaluation is enqueued on that assumption; the device compares the new ranking metric with the one
    // that walk was sorted from (d_rank_used) and energy_end() repeats the call the slow way if they differ
    DevBuf<double> d_rank_used;
    DevBuf<unsigned int> d_rankcnt;       // neighbour counters of the ranking metric
    std::vector<double> rank_saved;       // host copy of the metric d_rank_used holds (download_ranking sorts it on demand)
    bool perm_ranked = false;             // the last call's sweeps used the ranked walk
    bool rank_used_valid = false;
    bool force_host_rank = false;         // while energy_end() repeats a speculative call: no speculation
    unsigned long long spec_redos = 0;
    // ---- grand-canonical slots (insert_molecule / remove_molecule): c->n is the number of atom SLOTS in use,
    // some of which may be holes left by removed molecules
    int n_valid = 0;                     // atoms actually present
    int next_mol = 0;                    // next unused molecule id
    std::vector<char> slot_valid;        // per atom slot
    std::vector<char> slot_polar;        // per atom slot: polarizability != 0 (what a stated sweep order must cover exactly)
    std::vector<std::pair<int, int>> holes;  // (first, count) of removed molecules, reusable by an insert of that size
    std::vector<int> lrc_dirty_atoms;    // atoms inserted / removed since the static sums (the long-range corrections, rd_crystal's
                                         // self part) were made: ONE list, read by every such sum of a call, cleared once behind them
    int n_mol_uploaded = 0;         // molecules of the last upload (their ids are 0 .. n_mol_uploaded - 1)
    bool edited = false;            // insert_molecule / remove_molecule since the last upload: ids no longer in upload order
    // Gauss-Seidel + grand-canonical edits: the sweep ORDER is part of the result, and after insert / remove the
    // engine's slot order is no longer the caller's atom order.  The caller then states the order of the polarizable
    // sites (mpmc_hip_set_sweep_order); until it has, energy() refuses to run.
    bool order_stale = false;
    // ---- resident-solver fallback
    bool resident_off = false;             // a resident launch gave up: this context keeps to the multi-launch path ...
    long resident_retry_at = 0;            // ... until this many energy() calls have been made (then it tries once more),
    long resident_backoff = 0;             // the interval doubling with every further give-up (4 096 ... 1 048 576 calls)
    bool force_multi_launch = false;       // while energy_end() repeats a call whose resident launch gave up
    bool res_attr_set = false;
    unsigned long long resident_calls = 0, resident_fallbacks = 0;
    // ---- one MC step as a HIP graph (see graph_step())
    int graph_mode = 0;                  // GM_DIRECT | GM_CAPTURE | GM_UPDATE
    StepGraph sg;
    int eligible_streak = 0;             // consecutive calls that met graph_eligible()
    unsigned long long graph_launches = 0;
    double graph_update_s = 0.0, graph_launch_s = 0.0;
    // ---- staging and pinned buffers
    PinnedBuf<int> h_dirty;         // pinned staging for dirty slots
    PinnedBuf<double> h_stage;      // pinned staging ring for update_atoms() coordinates and scale_box() displacements
    size_t stage_used = 0;
    DevBuf<double> d_delta;         // scale_box(): per-molecule displacements [n_molecules][3]
    DevBuf<double> d_res;     // R_COUNT doubles
    PinnedBuf<double> h_res;  // pinned, mapped
    double *h_res_dev = nullptr;
    PinnedBuf<double> h_res2;  // the side stream's part of the record (LJ / Ewald sums) with a sequence number of its own
    double *h_res2_dev = nullptr;
    PinnedBuf<unsigned long long> h_err;  // pinned, 1 word
    PinnedBuf<unsigned> h_gserr;          // pinned: error words of the persistent Gauss-Seidel kernel (2 views)
    PinnedBuf<int> h_order;               // pinned staging of set_sweep_order (2 x max_npad ints)
    PinnedBuf<double> h_rank;             // pinned, max_npad
    PinnedBuf<int> h_perm;                // pinned, max_npad
    PinnedBuf<int> h_slotmap;             // pinned, max_npad: an atom -> slot map on its way to the device
    // ---- timing
    std::vector<HipEvent> ev_pool;
    size_t ev_next = 0;             // of the call in progress: begin_call() rewinds the pool and clears the records, whose
    std::vector<TimeRec> recs;      //     storage is kept from call to call (get_timings reads them after energy_end)
    HipEvent ev_first, ev_last;
    bool timed = false;
    double host_enqueue_s = 0.0, host_wait_s = 0.0;  // MPMC_HIP_HOST_PROFILE=1: printed at destroy
};

static DevAtoms dev_atoms(const mpmc_hip_ctx *c) {
    DevAtoms a;
    a.x = c->d_x;
    a.y = c->d_y;
    a.z = c->d_z;
    a.q = c->d_q;
    a.alpha = c->d_alpha;
    a.eps = (c->disp_on || c->rdc_order || c->vdw_on || c->rd_form) ? c->d_zero : c->d_eps;
    a.sig = (c->disp_on || c->rdc_order || c->vdw_on || c->rd_form) ? c->d_zero : c->d_sig;
    a.molmass = c->d_molmass;
    a.mol = c->d_mol;
    a.flags = c->d_flags;
    a.n = c->n;
    a.npad = c->npad;
    return a;
}
// `a` with the real epsilon / sigma whatever the mode: what the kernels of rd_crystal, set_rd_form and polarvdw read
static DevAtoms lj_atoms(const mpmc_hip_ctx *c, DevAtoms a) {
    a.eps = c->d_eps;
    a.sig = c->d_sig;
    return a;
}

static DevBox dev_box(const mpmc_hip_ctx *c) {
    DevBox b;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
            b.b[p][q] = c->basis[p][q];
            b.rb[p][q] = c->recip[p][q];
        }
    b.cutoff = c->cutoff;
    b.volume = c->volume;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
            b.fb[p][q] = (float)c->basis[p][q];
            b.frb[p][q] = (float)c->recip[p][q];
        }
    b.rc2_pre = (float)((c->cutoff + 0.01) * (c->cutoff + 0.01));
    b.screen64 = (c->coord_max > kScreen32MaxCoord || !(c->coord_max == c->coord_max)) ? 1 : 0;
    // half-integer guard of the screens (device_common.h): bound on the error of a fractional displacement
    double smax = 0.0, rmax = 0.0;
    for (int q = 0; q < 3; ++q) {
        smax = std::max(smax, std::fabs(c->recip[0][q]) + std::fabs(c->recip[1][q]) + std::fabs(c->recip[2][q]));
        for (int p = 0; p < 3; ++p) rmax = std::max(rmax, std::fabs(c->recip[p][q]));
    }
    const float tie32 = (float)(1.25 * 11.0 * 0x1p-13 * smax);
    b.half_tie32 = 0.5f - tie32;  // (NaN basis: the comparison is false and the distance test's NaN rule decides)
    b.tie64 = 0x1p-49 * rmax;
    b.tie_guard = c->box_ortho ? 0 : 1;
    return b;
}

// The dipole tensor's model and its parameters (kernels_polar.h).  `idx`: the atom of each slot when the kernel's atom
// set is a sweep view, nullptr when it is the configuration.  The Wolf constants are those of the current box: every
// launch forms them anew, so a box change needs no bookkeeping beyond the rebuild it already causes.
static int thole_model_of(const mpmc_hip_ctx *c) {
    if (c->thole_damp_type == 0) return kTholeOff;
    if (c->thole_damp_type == 1) return kTholeLinear;
    return c->thole_wolf_full ? kTholeExpWolf : kTholeExp;
}
static TholeParams thole_params(const mpmc_hip_ctx *c, const int *idx) {
    TholeParams tp;
    tp.damp = c->par.polar_damp;
    tp.rc = c->cutoff;
    tp.irc3 = tp.wdamp1 = tp.wdamp2 = 0.0;
    tp.idx = nullptr;
    const int model = thole_model_of(c);
    if (model == kTholeOff) tp.idx = idx;
    if (model == kTholeExpWolf) {  // thole_matrix.c:44-53, :113-114
        const double l = tp.damp, l2 = l * l, l3 = l2 * l, rc = tp.rc, rc2 = rc * rc, rc3 = rc2 * rc;
        const double explrcut = std::exp(-l * rc);
        tp.wdamp1 = 1.0 - explrcut * (0.5 * l2 * rc2 + l * rc + 1.0);
        tp.wdamp2 = tp.wdamp1 - explrcut * (l3 * rc3 / 6.0);
        tp.irc3 = 1.0 / rc3;
    }
    return tp;
}
// KERNEL<MODEL> for the context's model: every model is an instantiation of its own, the exponential one today's code
#define MPMC_THOLE_DISPATCH(c, ...)                                                   \
    do switch (thole_model_of(c)) {                                                   \
        case kTholeLinear: { constexpr int kM = kTholeLinear; __VA_ARGS__; break; }   \
        case kTholeOff: { constexpr int kM = kTholeOff; __VA_ARGS__; break; }         \
        case kTholeExpWolf: { constexpr int kM = kTholeExpWolf; __VA_ARGS__; break; } \
        default: { constexpr int kM = kTholeExp; __VA_ARGS__; break; }                \
    } while (0)

static int complete_pending_sweep(mpmc_hip_ctx *c);  // engine_polar.inc
template <int NRHS>
static int exact_substitute(mpmc_hip_ctx *c, int nv, int nvpad, const double *es);  // engine_polar.inc
// the polarization result is gone (the configuration it belongs to is being replaced): nobody can ask for the pending sweep
static void drop_polar_result(mpmc_hip_ctx *c) {
    c->psweep.drop();
    c->have_polar_result = false;
}
static void (*chain_kernel_of(int ortho))(GsChain);  // engine_polar.inc

// running maximum of |coordinate| (device_common.h: above kScreen32MaxCoord the pair / field screens switch
// from fp32 to fp64 displacements); a NaN coordinate switches too
static void note_coords(mpmc_hip_ctx *c, const double *x, const double *y, const double *z, int count) {
    double m = c->coord_max;
    for (int i = 0; i < count; ++i) {
        const double v = std::max(std::fabs(x[i]), std::max(std::fabs(y[i]), std::fabs(z[i])));
        if (!(v <= m)) m = (v == v) ? v : INFINITY;
    }
    const bool was64 = c->coord_max > kScreen32MaxCoord;
    c->coord_max = m;
    if ((m > kScreen32MaxCoord) != was64) ++c->config_rev;  // a captured step graph carries the old DevBox
}

// timing 1: events around the sweep kernels of every 32nd call (an event pair costs ~5 us of stream time and
// reading the events back stalls the host: sampling every 8th call cost 10 % of the step rate); 2: every call;
// -1: only the first-launch / last-kernel pair of every 32nd call (length of the device chain)
static inline bool is_timed_call(const mpmc_hip_ctx *c) {
    return c->opt.timing >= 2 || ((c->opt.timing == 1 || c->opt.timing == -1) &&
                                 (c->energy_calls % (unsigned long long)c->opt.timing_interval) == 0ull);
}

// Launch of one of the GraphSlotId kernels: a plain launch (which stream capture records), or, while a
// step graph is being refreshed, an update of that kernel's node in the instantiated graph.
template <typename... KArgs, typename... Args, size_t... I>
static hipError_t launch_slot_impl(mpmc_hip_ctx *c, int slot, void (*kernel)(KArgs...), dim3 g, dim3 b, hipStream_t s,
                                   std::index_sequence<I...>, Args &&...args) {
    std::tuple<KArgs...> vals(std::forward<Args>(args)...);
    void *argv[] = {(void *)&std::get<I>(vals)...};
    if (c->graph_mode == GM_UPDATE) {
        hipKernelNodeParams p;
        memset(&p, 0, sizeof(p));
        p.func = (void *)kernel;
        p.gridDim = g;
        p.blockDim = b;
        p.sharedMemBytes = 0;
        p.kernelParams = argv;
        p.extra = nullptr;
        return hipGraphExecKernelNodeSetParams(c->sg.exec, c->sg.node[slot], &p);
    }
    c->sg.func[slot] = (void *)kernel;
    return hipLaunchKernel((const void *)kernel, g, b, argv, 0, s);
}
template <typename... KArgs, typename... Args>
static hipError_t launch_slot(mpmc_hip_ctx *c, int slot, void (*kernel)(KArgs...), dim3 g, dim3 b, hipStream_t s,
                              Args &&...args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "argument count");
    return launch_slot_impl(c, slot, kernel, g, b, s, std::index_sequence_for<KArgs...>{}, std::forward<Args>(args)...);
}

struct ScopedTimer {
    mpmc_hip_ctx *c;
    hipStream_t s;
    TimeRec r;
    bool on;
    ScopedTimer(mpmc_hip_ctx *ctx, int cls, hipStream_t st = nullptr) : c(ctx), s(st ? st : ctx->stream), on(false) {
        const bool wanted = c->graph_mode == GM_DIRECT &&
                            (c->opt.timing >= 2 ||
                             (c->opt.timing == 1 && (cls == T_SWEEP || cls == T_EVPAIR) && is_timed_call(c)));
        if (wanted && c->ev_next + 2 <= c->ev_pool.size()) {
            r.cls = cls;
            r.a = c->ev_pool[c->ev_next++];
            r.b = c->ev_pool[c->ev_next++];
            hipEventRecord(r.a, s);
            on = true;
        }
    }
    ~ScopedTimer() {
        if (on) {
            hipEventRecord(r.b, s);
            c->recs.push_back(r);
        }
    }
};

// Launch of a kernel whose duration is to be reported (the roofline probe of bench.py): on a timed call the
// kernel is launched with hipExtLaunchKernel and a start / stop event pair, which carry the dispatch's OWN begin /
// end timestamps (what rocprofv3's kernel trace reads) -- an event pair recorded around a launch on the stream
// also counts ~3-5 us of marker processing, a quarter of a 17 us kernel.  Otherwise a plain launch.
template <typename... KArgs, typename... Args>
static hipError_t launch_timed(mpmc_hip_ctx *c, int cls, void (*kernel)(KArgs...), dim3 g, dim3 b, unsigned shmem,
                               hipStream_t s, Args &&...args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "argument count");
    std::tuple<KArgs...> vals(std::forward<Args>(args)...);
    void *argv[sizeof...(KArgs)];
    {
        size_t k = 0;
        std::apply([&](auto &...v) { ((argv[k++] = (void *)&v), ...); }, vals);
    }
    const bool wanted = c->graph_mode == GM_DIRECT &&
                        (c->opt.timing >= 2 || (c->opt.timing == 1 && cls == T_SWEEP && is_timed_call(c)));
    if (wanted && c->ev_next + 2 <= c->ev_pool.size()) {
        TimeRec r;
        r.cls = cls;
        r.a = c->ev_pool[c->ev_next++];
        r.b = c->ev_pool[c->ev_next++];
        const hipError_t e = hipExtLaunchKernel((const void *)kernel, g, b, argv, shmem, s, r.a, r.b, 0);
        if (e == hipSuccess) c->recs.push_back(r);
        return e;
    }
    return hipLaunchKernel((const void *)kernel, g, b, argv, shmem, s);
}

// The options of mpmc_hip_set_option(), in the order of the comment in include/mpmc_hip.h.  A row with a hook does more
// than store the value: the hook stores it itself (and may refuse it: -1).
struct OptionRow {
    const char *name;
    int EngineOptions::*member;
    int (*hook)(mpmc_hip_ctx *c, int value);
};
static const OptionRow kOptions[] = {
    // (the resident data were made the other way)
    {"pair_coefficients", &EngineOptions::pair_coef, [](mpmc_hip_ctx *c, int v) { c->opt.pair_coef = v; c->all_dirty = true; return 0; }},
    {"incremental_amatrix", &EngineOptions::incremental, [](mpmc_hip_ctx *c, int v) { c->opt.incremental = v; c->all_dirty = true; return 0; }},
    {"incremental_pairs", &EngineOptions::incremental_pairs,
     [](mpmc_hip_ctx *c, int v) { c->opt.incremental_pairs = v; c->all_dirty = true; return 0; }},
    {"overlap_streams", &EngineOptions::overlap, nullptr},
    {"side_after", &EngineOptions::side_after, [](mpmc_hip_ctx *c, int v) { c->opt.side_after = std::max(1, v); return 0; }},
    {"symmetric_sweep", &EngineOptions::symmetric, nullptr},
    {"sym_mode", &EngineOptions::sym_mode, nullptr},
    {"timing", &EngineOptions::timing, nullptr},
    {"timing_interval", &EngineOptions::timing_interval,
     [](mpmc_hip_ctx *c, int v) { c->opt.timing_interval = std::max(1, v); return 0; }},
    {"persistent_gs", &EngineOptions::persistent_gs, nullptr},
    {"speculative_ranking", &EngineOptions::spec_rank, nullptr},
    {"fuse_tensor", &EngineOptions::fuse_tensor, nullptr},
    {"gs_lags", &EngineOptions::gs_lags,
     [](mpmc_hip_ctx *c, int v) {
         if (v < 2 || v > kGsMaxLag) return fail("mpmc_hip_set_option: gs_lags must be 2 .. %d", kGsMaxLag);
         if (v != c->opt.gs_lags) c->view[0].M_epoch = c->view[1].M_epoch = 0;  // (the matrices of the new lags are not there)
         c->opt.gs_lags = v;
         return 0;
     }},
    {"gs_build_fork", &EngineOptions::gs_build_fork, nullptr},
    {"gs_side_waves", &EngineOptions::gs_side_waves, [](mpmc_hip_ctx *c, int v) { c->opt.gs_side_waves = (v == 16) ? 16 : 0; return 0; }},
    {"rank_view_side", &EngineOptions::rank_view_side, nullptr},
    {"gs_fold_upper", &EngineOptions::gs_fold_upper, nullptr},
    {"gs_fold_finish", &EngineOptions::gs_fold_finish, nullptr},
    {"rank_late", &EngineOptions::rank_late, nullptr},
    {"resident_jacobi", &EngineOptions::resident,
     [](mpmc_hip_ctx *c, int v) {
         c->opt.resident = v;  // 0: one sweep + one finish launch per iteration (A/B; bit-identical results)
         if (v) c->resident_off = false;
         return 0;
     }},
    {"resident_fold", &EngineOptions::res_fold, nullptr},
    {"resident_side", &EngineOptions::res_side, nullptr},
    {"sweep_alternate", &EngineOptions::sweep_alternate, nullptr},
    {"sweep_nt", &EngineOptions::sweep_nt, nullptr},
    {"sweep_split", &EngineOptions::sweep_split, nullptr},
    {"fuse_moves", &EngineOptions::fuse_moves, nullptr},
    {"gs_fuse_moves", &EngineOptions::gs_fuse_moves, nullptr},
    {"fuse_field", &EngineOptions::fuse_field, nullptr},
    {"fuse_recip", &EngineOptions::fuse_recip, nullptr},
    {"split_record", &EngineOptions::split_record, nullptr},
    {"side_moves", &EngineOptions::side_moves, nullptr},
    {"resident_stamps", &EngineOptions::res_stamps, nullptr},
    {"sweep_ablate", &EngineOptions::sweep_ablate, nullptr},
    {"resident_fault", &EngineOptions::res_fault, nullptr},
    {"gs_stamps", &EngineOptions::gs_stamps, nullptr},
    {"inv_stamps", &EngineOptions::inv_stamps, nullptr},
    {"gs_ablate", &EngineOptions::gs_ablate, nullptr},
    {"gs_fault_sweep", &EngineOptions::gs_fault_sweep, nullptr},
    {"step_graph", &EngineOptions::graph, nullptr},
};

extern "C" int mpmc_hip_set_option(mpmc_hip_ctx *c, const char *name, int value) {
    if (!c || !name) return fail("MPMC_HIP: set_option: null argument");
    // The cavity grid's knob is state of that grid, not of an evaluation: kOptions below holds the knobs of energy(), whose
    // change completes pending sweeps and retires a captured step; this one touches neither.
    if (!strcmp(name, "cavity_incremental")) {
        c->cav_incremental = value;
        return 0;
    }
    // Likewise the path of mpmc_hip_trial_energies(): no evaluation reads it, so setting it completes no pending sweep and
    // leaves config_rev -- and with it the "completed energy() on the current configuration" the entry asks for -- alone.
    if (!strcmp(name, "trial_batched")) {
        c->trial_batched = value;
        return 0;
    }
    if (complete_pending_sweep(c)) return -1;  // (launched under the options of the call it belongs to)
    ++c->config_rev;
    for (const OptionRow &o : kOptions) {
        if (strcmp(name, o.name)) continue;
        if (o.hook) return o.hook(c, value);
        c->opt.*o.member = value;
        return 0;
    }
    return fail("MPMC_HIP: set_option: unknown option '%s'", name);
}

extern "C" void mpmc_hip_default_params(mpmc_hip_params *p) {
    memset(p, 0, sizeof(*p));
    p->rd_lrc = 1;           // reference src/io/input.c:1630
    p->ewald_kmax = 7;       // defines.h:61
    p->polar_gamma = 1.0;    // input.c:1625
    p->polar_max_iter = 10;  // input.c:1626
    p->feynman_hibbs_order = 2;
}

extern "C" int mpmc_hip_create(mpmc_hip_ctx **out, int device, int max_atoms) {
    if (!out || max_atoms <= 0) return fail("MPMC_HIP: create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("MPMC_HIP: no HIP device available (this engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("MPMC_HIP: device %d out of range (%d present)", device, ndev);
    (void)hipSetDeviceFlags(hipDeviceScheduleSpin);  // low wake-up latency on the per-step synchronisation
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("MPMC_HIP: device %d is %s; this engine is built for gfx950 (MI355X) only", device,
                    prop.gcnArchName);
    std::unique_ptr<mpmc_hip_ctx> owner(new mpmc_hip_ctx());  // (an early return below frees what was made)
    mpmc_hip_ctx *c = owner.get();
    c->device = device;
    c->max_atoms = max_atoms;
    c->max_npad = round_up(max_atoms, 128);
    mpmc_hip_default_params(&c->par);
    const size_t np = (size_t)c->max_npad;
    c->num_cus = prop.multiProcessorCount;
    for (int o = 0; o < 2; ++o)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(chain_kernel_of(o)),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kChainLds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gs_block_inverse_kernel<0, 4>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kInverseLds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gs_block_inverse_kernel<1, 4>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kInverseLds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gs_block_inverse_kernel<0, 8>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kInverseLds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gs_block_inverse_kernel<1, 8>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kInverseLds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gs_block_inverse_kernel<0, 16>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kInverseLds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gs_block_inverse_kernel<1, 16>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kInverseLds));
    /* Two priority classes, so that the two streams never share a hardware queue whatever other streams
     * the process holds (the runtime pools its queues per priority; with RCCL initialised first both
     * streams otherwise land on one queue and the LJ/Ewald overlap is lost).  The polarization chain is
     * the critical path and takes the higher priority. */
    int prio_least = 0, prio_greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    HIPCHK(hipStreamCreateWithPriority(c->stream.out(), hipStreamNonBlocking, prio_greatest));
    HIPCHK(hipStreamCreateWithPriority(c->stream2.out(), hipStreamNonBlocking, prio_least));
    HIPCHK(hipStreamCreateWithPriority(c->stream3.out(), hipStreamNonBlocking, prio_greatest));
    HIPCHK(hipEventCreateWithFlags(c->ev_bfork.out(), hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(c->ev_bjoin.out(), hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(c->ev_fork.out(), hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(c->ev_join.out(), hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(c->ev_rank.out(), hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(c->ev_order.out(), hipEventDisableTiming));
    HIPCHK(c->d_x.alloc(np));
    HIPCHK(c->d_y.alloc(np));
    HIPCHK(c->d_z.alloc(np));
    HIPCHK(c->d_q.alloc(np));
    HIPCHK(c->d_alpha.alloc(np));
    HIPCHK(c->d_eps.alloc(np));
    HIPCHK(c->d_sig.alloc(np));
    HIPCHK(c->d_molmass.alloc(np));
    HIPCHK(c->d_mol.alloc(np));
    HIPCHK(c->d_flags.alloc(np));
    HIPCHK(c->d_es.alloc(3 * np));
    HIPCHK(c->d_mu.alloc(3 * np));
    HIPCHK(c->d_efind.alloc(3 * np));
    HIPCHK(c->d_efchg.alloc(3 * np));
    HIPCHK(c->d_tmp3.alloc(3 * np));
    HIPCHK(c->d_rank.alloc(np));
    HIPCHK(c->d_rank_used.alloc(np));
    HIPCHK(c->d_rankcnt.alloc(np));
    HIPCHK(c->d_errmax.alloc(256));
    for (SweepView &v : c->view) {
        v.cap = (int)np;
        HIPCHK(v.d_idx.alloc(np));
        HIPCHK(v.d_slot.alloc(np));
        HIPCHK(v.px.alloc(np));
        HIPCHK(v.py.alloc(np));
        HIPCHK(v.pz.alloc(np));
        HIPCHK(v.palpha.alloc(np));
        HIPCHK(v.pflags.alloc(np));
        HIPCHK(v.es.alloc(3 * np));
        HIPCHK(v.mu0.alloc(3 * np));
        HIPCHK(v.mu1.alloc(3 * np));
        HIPCHK(v.munew.alloc(3 * np));
        HIPCHK(v.mupub.alloc(kGsMaxLag * (3 * np + 192)));  // mu_t of a sweep, then (gs_qoff apart) the auxiliary lags' vectors; a spare block each
        c->gs_qoff = (int)(3 * np + 192);
        HIPCHK(v.y.alloc(3 * np));
        HIPCHK(v.efind.alloc(3 * np));
        HIPCHK(v.tmu0.alloc(3 * np));
        HIPCHK(v.efchg.alloc(3 * np));
        HIPCHK(v.rrms.alloc(np));
        HIPCHK(v.gsflags.alloc(16));
        HIPCHK(hipMemsetAsync(v.gsflags, 0, 16 * sizeof(unsigned), c->stream));
        HIPCHK(v.energy_part.alloc(2 * (np / 64 + 1)));
        // slots past the last tile of a view are never written by the tiled sweep: keep them defined
        for (double *p : {v.mu0.get(), v.mu1.get(), v.munew.get(), v.y.get(), v.efind.get(), v.efchg.get(), v.es.get()})
            HIPCHK(hipMemsetAsync(p, 0, 3 * np * sizeof(double), c->stream));
        HIPCHK(hipMemsetAsync(v.rrms, 0, np * sizeof(double), c->stream));
    }
    const size_t ntile = np / 64;
    HIPCHK(c->d_pairpart.alloc(ntile * ntile * kPairChannels));
    HIPCHK(c->lrc.part.alloc(ntile * ntile));
    HIPCHK(c->d_rankpart.alloc(ntile * ntile));
    const size_t nchunk_max = std::max<size_t>(1, np / 64) + 16;  // + k-chunk slots of the Ewald field
    HIPCHK(c->d_fieldpart.alloc(nchunk_max * 3 * np));
    HIPCHK(c->d_res.alloc(R_COUNT));
    HIPCHK(c->h_res.alloc(R_COUNT + 1, hipHostMallocMapped));
    c->h_res[R_COUNT] = 0.0;
    HIPCHK(hipHostGetDevicePointer((void **)&c->h_res_dev, c->h_res, 0));
    HIPCHK(c->h_res2.alloc(R_COUNT + 1, hipHostMallocMapped));
    memset(c->h_res2, 0, (R_COUNT + 1) * sizeof(double));
    HIPCHK(hipHostGetDevicePointer((void **)&c->h_res2_dev, c->h_res2, 0));
    HIPCHK(c->h_err.alloc(1));
    HIPCHK(c->h_gserr.alloc(2));
    HIPCHK(c->h_rank.alloc(np));
    HIPCHK(c->h_perm.alloc(np));
    HIPCHK(c->h_slotmap.alloc(np));
    HIPCHK(c->h_dirty.alloc(kMaxDirty));
    HIPCHK(c->h_stage.alloc(3 * 4096));
    c->ev_pool.resize(2 * 512);
    for (auto &e : c->ev_pool) HIPCHK(hipEventCreate(e.out()));
    HIPCHK(hipEventCreate(c->ev_first.out()));
    HIPCHK(hipEventCreate(c->ev_last.out()));
    HIPCHK(hipMemsetAsync(c->d_res, 0, R_COUNT * sizeof(double), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (device < 64) ++g_ctx_on_device[device];
    *out = owner.release();
    return 0;
}

static void graph_destroy(mpmc_hip_ctx *c);

// the context's members free its buffers, streams and events
extern "C" void mpmc_hip_destroy(mpmc_hip_ctx *c) {
    if (!c) return;
    if (getenv("MPMC_HIP_HOST_PROFILE") && c->energy_calls)
        fprintf(stderr, "MPMC_HIP host profile: %llu energy() calls (%llu as graph), enqueue %.1f us, wait %.1f us per call\n",
                c->energy_calls, c->graph_launches, 1e6 * c->host_enqueue_s / c->energy_calls,
                1e6 * c->host_wait_s / c->energy_calls);
    if (getenv("MPMC_HIP_HOST_PROFILE") && c->graph_launches)
        fprintf(stderr, "MPMC_HIP graph steps: node updates %.1f us, launch %.1f us per step\n",
                1e6 * c->graph_update_s / c->graph_launches, 1e6 * c->graph_launch_s / c->graph_launches);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->stream2);
    hipStreamSynchronize(c->stream3);
    graph_destroy(c);
    if (c->device < 64) --g_ctx_on_device[c->device];
    delete c;
}

// ---- What an event makes stale; DESIGN.md ("Tile passes") has the table and the reasons.  The mode setters
// (engine_dense.inc) drop their own term's sums where they stand.
// all_dirty, or the moved blocks cannot be listed: every sum over positions (the static ones read no coordinate)
static void positions_unknown(mpmc_hip_ctx *c) {
    c->pair_part_valid = c->field_part_valid = c->disp.valid = c->rdc.valid = c->at.valid = false;
    c->rep.valid = c->vdw.valid = c->rdf.valid = false;
}
// set_params(), or an insertion grew the tile grid (grid_grew()).  Not c->at: no parameter enters the three-body term; a
// full triple pass after every set_params() would be wasted.
static void params_or_grid_changed(mpmc_hip_ctx *c) {
    c->pair_part_valid = c->field_part_valid = c->disp.valid = c->rdc.valid = false;
    c->rep.valid = c->vdw.valid = false;  // (polar_damp enters the matrix)
    c->rdf.valid = false;
}
// An appended molecule changed npad: a tile's slot in every partial array is I * ntile + J and the count of three-body units
// follows ntile, so every tile sum, static ones included, is made from scratch.
static void grid_grew(mpmc_hip_ctx *c) {
    params_or_grid_changed(c);
    c->lrc.valid = c->disp_lrc.valid = c->rdf_lrc.valid = c->rdc_static.valid = c->at.valid = false;
}
// apply_box(): the sums of parameters, cutoff and volume (those over positions go with all_dirty)
static void box_changed(mpmc_hip_ctx *c) {
    c->lrc.valid = c->disp_lrc.valid = c->rdc_static.valid = c->rep_lrc.valid = c->vdw_lrc.valid = false;
    c->rdf_lrc.valid = false;
    c->cav_pos_valid = c->cav_occ_valid = false;  // the cavity grid's points are fractions of the cell
    c->cav_open = -1;
}
// upload(): everything per-atom (the pair / field partials go with all_dirty; the rd_crystal SETTING stays)
static void atoms_replaced(mpmc_hip_ctx *c) {
    c->lrc.valid = c->disp.valid = c->disp_lrc.valid = c->at.valid = c->rdc.valid = c->rdc_static.valid = false;
    c->rep.valid = c->rep_lrc.valid = c->vdw.valid = c->vdw_lrc.valid = false;
    c->rdf.valid = c->rdf_lrc.valid = false;
}

// reference src/io/check_input.c:318-470 (the subset that concerns this path)
extern "C" int mpmc_hip_set_params(mpmc_hip_ctx *c, const mpmc_hip_params *p) {
    if (!c || !p) return fail("MPMC_HIP: set_params: null argument");
    if (p->feynman_hibbs && p->feynman_hibbs_order != 2 && p->feynman_hibbs_order != 4)
        return fail("MPMC_HIP: feynman_hibbs_order must be 2 or 4");
    if (p->feynman_hibbs && !(p->temperature > 0.0)) return fail("MPMC_HIP: feynman_hibbs needs temperature > 0");
    if (p->ewald_kmax < 0 || p->ewald_kmax > 32) return fail("MPMC_HIP: ewald_kmax out of range");
    if (p->wolf && p->feynman_hibbs && !p->rd_only)
        return fail("MPMC_HIP: COULOMBIC: FH + es_wolf is not implemented");  // coulombic.c:294-298
    if (p->polarization) {
        // (check_input.c:406-409: not under polar_damp_type off, which reads no damping factor; energy() asks again
        //  should the model be switched back)
        if (!(p->polar_damp > 0.0) && c->thole_damp_type != 0) return fail("MPMC_HIP: damping factor must be specified (polar_damp > 0)");
        if (p->polar_precision > 0.0 && p->polar_max_iter > 0)
            return fail("MPMC_HIP: cannot specify both polar_precision and polar_max_iter, must pick one");
        if (p->polar_precision < 0.0) return fail("MPMC_HIP: invalid polarization iterative precision specified");
        // (the exact dipoles read no solver parameter: a set without either is accepted while that mode is on, and
        //  energy() refuses it should the mode be switched off again)
        if (p->polar_precision == 0.0 && p->polar_max_iter <= 0 && !p->polar_zodid && !c->exact_polar)
            return fail("MPMC_HIP: polar_max_iter must be > 0 when polar_precision is 0");
        if (p->polar_sor && p->polar_esor) return fail("MPMC_HIP: cannot specify both SOR and ESOR SCF methods");
        if (p->polar_gamma < 0.0) return fail("MPMC_HIP: invalid Pre-cond/SOR/ESOR gamma set");
    }
    if (complete_pending_sweep(c)) return -1;
    if (p->polar_damp != c->par.polar_damp) c->all_dirty = true;
    params_or_grid_changed(c);
    ++c->config_rev;
    c->par_user = *p;
    c->par = *p;
    if (c->rd_form == kRdFormSG) c->par.rd_only = 1;  // energy.c:108, :154: no electrostatics, no polarization under sg
    c->have_params = true;
    c->kvecf_valid = false;
    c->kvec_valid = false;
    return 0;
}

// reference src/energy/pbc.c:13-83; shared by set_box() and scale_box()
static int apply_box(mpmc_hip_ctx *c, const double basis[9], double pbc_cutoff) {
    double b[3][3];
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) b[p][q] = basis[3 * p + q];
    double vol = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1]);
    vol += b[0][1] * (b[1][2] * b[2][0] - b[1][0] * b[2][2]);
    vol += b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0]);
    if (!(vol > 0.0)) return fail("MPMC_HIP: invalid simulation box dimensions (volume %g)", vol);
    double cutoff = pbc_cutoff;
    if (cutoff == 0.0) {
        double short_mag = kMAXVALUE;
        for (int i = -5; i <= 5; i++)
            for (int j = -5; j <= 5; j++)
                for (int k = -5; k <= 5; k++) {
                    if (i == 0 && j == 0 && k == 0) continue;
                    double v[3];
                    for (int q = 0; q < 3; q++) v[q] = i * b[0][q] + j * b[1][q] + k * b[2][q];
                    const double mag = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                    if (mag < short_mag) short_mag = mag;
                }
        cutoff = 0.5 * short_mag;
    }
    if (!(cutoff > 0.0)) return fail("MPMC_HIP: invalid cutoff");
    const double iv = 1.0 / vol;
    double rb[3][3];
    rb[0][0] = iv * (b[1][1] * b[2][2] - b[1][2] * b[2][1]);
    rb[0][1] = iv * (b[0][2] * b[2][1] - b[0][1] * b[2][2]);
    rb[0][2] = iv * (b[0][1] * b[1][2] - b[0][2] * b[1][1]);
    rb[1][0] = iv * (b[1][2] * b[2][0] - b[1][0] * b[2][2]);
    rb[1][1] = iv * (b[0][0] * b[2][2] - b[0][2] * b[2][0]);
    rb[1][2] = iv * (b[0][2] * b[1][0] - b[0][0] * b[1][2]);
    rb[2][0] = iv * (b[1][0] * b[2][1] - b[1][1] * b[2][0]);
    rb[2][1] = iv * (b[0][1] * b[2][0] - b[0][0] * b[2][1]);
    rb[2][2] = iv * (b[0][0] * b[1][1] - b[0][1] * b[1][0]);
    memcpy(c->basis, b, sizeof(b));
    memcpy(c->recip, rb, sizeof(rb));
    c->pbc_cutoff_in = pbc_cutoff;
    c->cutoff = cutoff;
    c->volume = vol;
    c->have_box = true;
    ++c->config_rev;
    c->box_ortho = (b[0][1] == 0.0 && b[0][2] == 0.0 && b[1][0] == 0.0 && b[1][2] == 0.0 && b[2][0] == 0.0 &&
                    b[2][1] == 0.0);
    c->kvecf_valid = false;
    c->kvec_valid = false;
    box_changed(c);
    c->all_dirty = true;
    return 0;
}

extern "C" int mpmc_hip_set_box(mpmc_hip_ctx *c, const double basis[9], double pbc_cutoff) {
    if (!c || !basis) return fail("MPMC_HIP: set_box: null argument");
    if (c->in_flight) return fail("MPMC_HIP: set_box between energy_begin() and energy_end()");
    if (complete_pending_sweep(c)) return -1;
    return apply_box(c, basis, pbc_cutoff);
}

extern "C" int mpmc_hip_upload(mpmc_hip_ctx *c, int n, const double *x, const double *y, const double *z,
                               const double *charge, const double *polarizability, const double *epsilon,
                               const double *sigma, const double *mass, const int *molecule,
                               const uint8_t *frozen) {
    if (!c) return fail("MPMC_HIP: upload: null context");
    if (c->in_flight) return fail("MPMC_HIP: upload between energy_begin() and energy_end()");
    if (n <= 0 || n > c->max_atoms) return fail("MPMC_HIP: upload: n = %d outside (0, %d]", n, c->max_atoms);
    if (!x || !y || !z || !charge || !polarizability || !epsilon || !sigma || !mass || !molecule || !frozen)
        return fail("MPMC_HIP: upload: null array");
    HIPCHK(hipSetDevice(c->device));
    drop_polar_result(c);
    const int npad = round_up(n, 128);
    const int nall = c->max_npad;  // every allocated slot is (re)initialised: later inserts may grow into them
    std::vector<double> hx(nall, 0.0), hy(nall, 0.0), hz(nall, 0.0), hq(nall, 0.0), ha(nall, 0.0), he(nall, 0.0),
        hs(nall, 0.0), hm(nall, 0.0);
    std::vector<int> hmol(nall, -1), hfl(nall, 0);
    int m = -1;
    for (int i = 0; i < n; ++i) {
        if (i == 0 || molecule[i] != molecule[i - 1]) ++m;  // contiguous runs, read_pqr.c:278-287
        hmol[i] = m;
        hx[i] = x[i];
        hy[i] = y[i];
        hz[i] = z[i];
        hq[i] = charge[i];
        ha[i] = polarizability[i];
        he[i] = epsilon[i];
        hs[i] = sigma[i];
        hfl[i] = kValid | (frozen[i] ? kFrozen : 0);
    }
    for (int s = 0; s < n;) {  // molecule mass = sum of its atoms' masses (update_com, pairs.c:364-385)
        int e = s;
        double mm = 0.0;
        while (e < n && hmol[e] == hmol[s]) mm += mass[e++];
        for (int i = s; i < e; ++i) hm[i] = mm;
        s = e;
    }
    // pad atoms: distinct molecule ids, far away; never valid
    for (int i = n; i < nall; ++i) hmol[i] = -2 - i;
    const size_t bd = nall * sizeof(double), bi = nall * sizeof(int);
    HIPCHK(hipMemcpyAsync(c->d_x, hx.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_y, hy.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_z, hz.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_q, hq.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_alpha, ha.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_eps, he.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_sig, hs.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_molmass, hm.data(), bd, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_mol, hmol.data(), bi, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_flags, hfl.data(), bi, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->coord_max = 0.0;
    note_coords(c, x, y, z, n);
    c->n = n;
    c->npad = npad;
    c->n_valid = n;
    c->next_mol = m + 1;
    c->n_mol_uploaded = m + 1;
    c->edited = false;
    c->slot_valid.assign(n, 1);
    c->slot_polar.assign(n, 0);
    for (int i = 0; i < n; ++i) c->slot_polar[i] = (polarizability[i] != 0.0);
    c->holes.clear();
    c->lrc_dirty_atoms.clear();
    c->self_valid = false;
    c->have_atoms = true;
    c->have_polar_result = false;
    c->disp_on = false;  // an upload brings Lennard-Jones parameters until set_dispersion() says otherwise
    c->at_on = false;  // ... and no three-body term until set_axilrod_teller() says otherwise
    c->chol_nv = 0;     // (the exact dipoles' factor was the old configuration's; the setting itself stays)
    c->vdw_on = false;  // ... and no coupled-dipole term until set_vdw() says otherwise (its e_iso cache stays for that call)
    c->negative_sigma = false;
    for (int i = 0; i < n; ++i) c->negative_sigma = c->negative_sigma || sigma[i] < 0.0;
    atoms_replaced(c);
    c->rank_saved.clear();
    c->perm_ranked = false;
    c->pending.n = 0;
    // view 0: polarizable atoms in atom order
    SweepView &v0 = c->view[0];
    v0.h_idx.clear();
    for (int i = 0; i < n; ++i)
        if (polarizability[i] != 0.0) v0.h_idx.push_back(i);
    v0.nv = (int)v0.h_idx.size();
    v0.nvpad = std::max(128, round_up(v0.nv, 128));
    v0.slot_of_atom.assign(n, -1);
    for (int k = 0; k < v0.nv; ++k) v0.slot_of_atom[v0.h_idx[k]] = k;
    {
        std::vector<int> hs(nall, -1);
        std::copy(v0.slot_of_atom.begin(), v0.slot_of_atom.end(), hs.begin());
        HIPCHK(hipMemcpy(v0.d_slot, hs.data(), nall * sizeof(int), hipMemcpyHostToDevice));
    }
    if (v0.C) {  // tiles beyond the ones the coming build rewrites must read as "no pair"
        HIPCHK(hipMemsetAsync(v0.C, 0, v0.C.size() * sizeof(double2), c->stream));
    }
    c->all_dirty = true;
    c->dirty_atoms.clear();
    c->view[0].A_valid = c->view[1].A_valid = false;
    c->view[0].C_valid = c->view[1].C_valid = false;
    c->view[0].pos_valid = c->view[1].pos_valid = false;
    c->rank_used_valid = false;
    c->order_stale = false;
    c->view[0].rebuild_from = c->view[1].rebuild_from = -1;
    ++c->config_rev;
    if (v0.nv > 0) HIPCHK(hipMemcpy(v0.d_idx, v0.h_idx.data(), v0.nv * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

static int flush_moves(mpmc_hip_ctx *c);
// The two three-body values of one site (AtAtoms): what set_axilrod_teller() stores for an uploaded atom and
// edit_molecules() for an inserted one.
static void at_site_values(double alpha, double c9, double &a, double &g) {
    a = alpha * kAtAlpha;
    // 1 / (c / p) with the reference's own p = pow(alpha * 6.7483345, 3) (axilrod_teller.cpp:121-122); c = 0 gives inf
    g = (a != 0.0) ? 1.0 / (c9 / std::pow(a, 3)) : 1.0;
}

// The exact dipoles (polar_iterative off, polar.c:91-95): A mu = E_static by a blocked Cholesky factorization on the device
// (kernels_exact.h) instead of an iterative solve.  A setting of the context, like set_rd_crystal().
extern "C" int mpmc_hip_set_exact_polar(mpmc_hip_ctx *c, int enable) {
    if (!c) return fail("MPMC_HIP: set_exact_polar: null context");
    if (c->in_flight) return fail("MPMC_HIP: set_exact_polar between energy_begin() and energy_end()");
    if ((enable != 0) == c->exact_polar) return 0;
    HIPCHK(hipSetDevice(c->device));
    if (complete_pending_sweep(c)) return -1;
    if (c->have_atoms && flush_moves(c)) return -1;  // keep the order of the caller's operations
    c->exact_polar = enable != 0;
    c->chol_nv = 0;
    c->chol_done = c->chol_failed = false;
    c->all_dirty = true;
    ++c->config_rev;
    return 0;
}

// The dipole tensor's model (thole_matrix.c:90-135; kernels_polar.h).  A setting of the context, like set_rd_crystal().
// Everything made from the tensor -- the coefficient store, the expanded matrix, the chain data, the Cholesky factor --
// goes with all_dirty; the static field's mode is part of its partials' key (launch_field()).
extern "C" int mpmc_hip_set_thole_model(mpmc_hip_ctx *c, const mpmc_hip_thole_model *m) {
    if (!c || !m) return fail("MPMC_HIP: set_thole_model: null argument");
    if (c->in_flight) return fail("MPMC_HIP: set_thole_model between energy_begin() and energy_end()");
    if (m->damp_type < 0 || m->damp_type > 2)
        return fail("MPMC_HIP: set_thole_model: damp_type %d outside 0 (off), 1 (linear), 2 (exponential)", m->damp_type);
    if (m->wolf_full && m->damp_type != 2)
        return fail("MPMC_HIP: set_thole_model: polar_wolf_full needs polar_damp_type exponential (damp_type 2)");
    const bool wolf_full = m->wolf_full != 0;
    if (m->damp_type == c->thole_damp_type && wolf_full == c->thole_wolf_full) return 0;  // nothing to change
    HIPCHK(hipSetDevice(c->device));
    if (complete_pending_sweep(c)) return -1;
    if (c->have_atoms && flush_moves(c)) return -1;  // keep the order of the caller's operations
    c->thole_damp_type = m->damp_type;
    c->thole_wolf_full = wolf_full;
    c->chol_nv = 0;
    c->chol_done = c->chol_failed = false;
    c->all_dirty = true;
    ++c->config_rev;
    return 0;
}

// The molecular polarizability tensor C[p][q] = sum_ij (A^-1)[3i+p][3j+q] (thole_polarizability.c:27-37), without the
// inverse: column q is the sum over the sites of the dipoles a unit field along q induces -- three more right-hand sides
// on the factor of the last completed energy().
extern "C" int mpmc_hip_get_polarizability_tensor(mpmc_hip_ctx *c, double out[9]) {
    if (!c || !out) return fail("MPMC_HIP: get_polarizability_tensor: null argument");
    if (c->in_flight) return fail("MPMC_HIP: get_polarizability_tensor between energy_begin() and energy_end()");
    if (!c->exact_polar)
        return fail("MPMC_HIP: get_polarizability_tensor: the exact dipoles are off (mpmc_hip_set_exact_polar; the reference: "
                    "iterative polarizability tensor method not implemented)");
    if (c->chol_nv <= 0 || !c->chol_done)
        return fail("MPMC_HIP: get_polarizability_tensor: no energy() with polarization has completed in this mode");
    if (c->chol_failed)
        return fail("MPMC_HIP: get_polarizability_tensor: the matrix of the last energy() was not positive definite");
    HIPCHK(hipSetDevice(c->device));
    if (exact_substitute<3>(c, c->chol_nv, c->chol_nvpad, nullptr)) return -1;
    hipLaunchKernelGGL(chol_tensor_kernel, dim3(1), dim3(256), 0, c->stream, c->chol_nv,
                       (const double *)(c->d_chol_vec + 6 * (size_t)(3 * c->chol_nvpad)), 3 * c->chol_nvpad,
                       c->d_chol_tensor.get());
    HIPCHK(hipMemcpyAsync(out, c->d_chol_tensor, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// apply the queued single-molecule moves (kept in order with any staged copies)
// What the side stream does before its first kernel that reads coordinates: apply the step's move itself (the same
// apply_moves_kernel with the same list: same bits into the same arrays as the main stream's launch; neither stream reads
// a moved coordinate before its own writer) -- or, when the move reached the device another way (edits, staged copies),
// wait for the event the main stream recorded behind it.
static void side_wait_for_moves(mpmc_hip_ctx *c, hipStream_t s);
// What the polarization chain (engine_polar.inc) calls at the points where the device has work queued: both do nothing
// outside the window enqueue_direct() opens for them, and nothing the second time.
static void feed_side_stream(mpmc_hip_ctx *c);  // the LJ / Ewald launches of the call (enqueue_side_stream)
static void publish_early(mpmc_hip_ctx *c);     // the publish launch, behind the finish that completes U_pol
static int flush_moves(mpmc_hip_ctx *c) {
    if (c->pending.n > 0) {
        // (outside an evaluation: a pending sweep reads the view's coordinates; energy_begin() has dropped it by now)
        if (complete_pending_sweep(c)) return -1;
        SweepView &v0 = c->view[0];
        HIPCHK(launch_slot(c, GS_MOVES, apply_moves_kernel, dim3(1), dim3(64), c->stream, c->pending, c->d_x, c->d_y,
                           c->d_z, v0.d_slot, v0.px, v0.py, v0.pz));
        c->pending.n = 0;
    }
    return 0;
}

static void side_wait_for_moves(mpmc_hip_ctx *c, hipStream_t s) {
    if (c->call.side_apply.n > 0) {
        SweepView &v0 = c->view[0];
        hipLaunchKernelGGL(apply_moves_kernel, dim3(1), dim3(64), 0, s, c->call.side_apply, c->d_x, c->d_y, c->d_z,
                           (const int *)v0.d_slot, v0.px, v0.py, v0.pz);
        c->call.side_apply.n = 0;
        c->call.side_applied = true;
        return;
    }
    if (c->call.side_applied) return;  // (already on this stream, earlier in the call)
    hipStreamWaitEvent(s, c->ev_fork, 0);
}

extern "C" int mpmc_hip_update_atoms(mpmc_hip_ctx *c, int first, int count, const double *x, const double *y,
                                     const double *z) {
    if (!c || !c->have_atoms) return fail("MPMC_HIP: update_atoms: no configuration uploaded");
    if (c->in_flight) return fail("MPMC_HIP: update_atoms between energy_begin() and energy_end()");
    if (first < 0 || count <= 0 || first + count > c->n)
        return fail("MPMC_HIP: update_atoms: range [%d, %d) outside [0, %d)", first, first + count, c->n);
    if (!x || !y || !z) return fail("MPMC_HIP: update_atoms: null array");
    HIPCHK(hipSetDevice(c->device));
    note_coords(c, x, y, z, count);
    const size_t b = count * sizeof(double);
    bool queued = false;
    if (count <= kMaxMoves) {
        // a single-molecule move: queue it for one argument-carried launch at the next energy()
        MoveList &m = c->pending;
        int need = 0;
        for (int i = 0; i < count; ++i) {
            bool found = false;
            for (int k = 0; k < m.n; ++k) found |= (m.idx[k] == first + i);
            need += !found;
        }
        if (m.n + need <= kMaxMoves) {
            for (int i = 0; i < count; ++i) {
                int slot = -1;
                for (int k = 0; k < m.n; ++k)
                    if (m.idx[k] == first + i) slot = k;
                if (slot < 0) slot = m.n++;
                m.idx[slot] = first + i;
                m.x[slot] = x[i];
                m.y[slot] = y[i];
                m.z[slot] = z[i];
            }
            queued = true;
        }
    }
    if (queued) {
        // nothing to launch yet
    } else if ((size_t)(3 * count) <= c->h_stage.size()) {
        if (complete_pending_sweep(c)) return -1;
        if (flush_moves(c)) return -1;
        c->staged_copies = true;
        c->main_writes = true;
        c->view[0].pos_valid = false;
        // small delta (one molecule): stage in pinned memory so the copies are truly asynchronous and the
        // caller's buffers are free at once; the ring is recycled after the next energy() has synchronised
        if (c->stage_used + 3 * (size_t)count > c->h_stage.size()) {
            HIPCHK(hipStreamSynchronize(c->stream));
            c->stage_used = 0;
        }
        double *s = c->h_stage + c->stage_used;
        memcpy(s, x, b);
        memcpy(s + count, y, b);
        memcpy(s + 2 * count, z, b);
        c->stage_used += 3 * (size_t)count;
        HIPCHK(hipMemcpyAsync(c->d_x + first, s, b, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_y + first, s + count, b, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_z + first, s + 2 * count, b, hipMemcpyHostToDevice, c->stream));
    } else {
        if (complete_pending_sweep(c)) return -1;
        if (flush_moves(c)) return -1;
        c->staged_copies = true;
        c->main_writes = true;
        c->view[0].pos_valid = false;
        HIPCHK(hipMemcpyAsync(c->d_x + first, x, b, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_y + first, y, b, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_z + first, z, b, hipMemcpyHostToDevice, c->stream));
        // pageable sources: make sure the copies are complete before the caller reuses its buffers
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (!c->all_dirty) {
        if ((int)c->dirty_atoms.size() + count > 4 * kMaxDirty)
            c->all_dirty = true;
        else
            for (int i = 0; i < count; ++i) c->dirty_atoms.push_back(first + i);
    }
    return 0;
}

// NPT volume move (mc_moves.c:168-210) and its revert (:213-248) on the resident configuration: the new box, and
// every molecule shifted rigidly by the displacement the host computed from its own centres of mass.  Nothing is
// uploaded again: the molecule table, the views' index arrays and slot maps and the coefficient store's padding stay;
// everything that is a function of the box or of all coordinates is marked for a rebuild by the next energy().
// Return 1 = the molecule ids are no longer those of the upload (grand-canonical edits): upload again.
extern "C" int mpmc_hip_scale_box(mpmc_hip_ctx *c, const double basis[9], double pbc_cutoff, int n_molecules,
                                  const double *delta) {
    if (!c || !basis || !delta) return fail("MPMC_HIP: scale_box: null argument");
    if (c->in_flight) return fail("MPMC_HIP: scale_box between energy_begin() and energy_end()");
    if (!c->have_atoms || !c->have_box) return fail("MPMC_HIP: scale_box: no configuration uploaded");
    if (c->edited || !c->holes.empty()) return 1;
    if (n_molecules != c->n_mol_uploaded)
        return fail("MPMC_HIP: scale_box: %d displacements for the %d molecules of the upload", n_molecules,
                    c->n_mol_uploaded);
    HIPCHK(hipSetDevice(c->device));
    const size_t need = 3 * (size_t)n_molecules;
    double dmax = 0.0;
    for (size_t k = 0; k < need; ++k) {
        const double v = std::fabs(delta[k]);
        if (!(v <= dmax)) dmax = (v == v) ? v : INFINITY;
    }
    if (complete_pending_sweep(c)) return -1;  // (a refused box below leaves the last result readable)
    if (flush_moves(c)) return -1;  // keep the order of the caller's operations
    if (c->d_delta.size() < need) {
        HIPCHK(hipStreamSynchronize(c->stream));  // (growth only: an earlier launch may still read the old buffer)
        HIPCHK(c->d_delta.alloc(need));
    }
    if (c->h_stage.size() < 2 * need) {  // room for a change and its revert between two energy() calls
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(c->h_stage.alloc(2 * need + 3 * 4096));
        c->stage_used = 0;
    }
    if (c->stage_used + need > c->h_stage.size()) {  // (as update_atoms: the ring is recycled after energy_end())
        HIPCHK(hipStreamSynchronize(c->stream));
        c->stage_used = 0;
    }
    if (apply_box(c, basis, pbc_cutoff)) return -1;  // (nothing enqueued yet: a refused box leaves the context as it was)
    double *s = c->h_stage + c->stage_used;
    memcpy(s, delta, need * sizeof(double));
    c->stage_used += need;
    HIPCHK(hipMemcpyAsync(c->d_delta, s, need * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SweepView &v0 = c->view[0];
    hipLaunchKernelGGL(shift_molecules_kernel, dim3((c->n + kShiftThreads - 1) / kShiftThreads), dim3(kShiftThreads), 0,
                       c->stream, c->n, n_molecules, (const double *)c->d_delta, (const int *)c->d_mol,
                       (const int *)c->d_flags, c->d_x.get(), c->d_y.get(), c->d_z.get(), (const int *)v0.d_slot,
                       v0.px.get(), v0.py.get(), v0.pz.get());
    HIPCHK(hipGetLastError());
    // |new coordinate| <= |old| + |delta|: the fp32 screen's guard holds without reading anything back.  The bound only
    // grows (a rejected volume move adds its shift twice for no net motion), so when it would cross the screen's limit
    // it is replaced once by the true maximum, read back from the device: the only case in which this call waits.
    {
        const bool was64 = c->coord_max > kScreen32MaxCoord;
        double bound = c->coord_max + dmax;
        if (!was64 && bound > kScreen32MaxCoord) {
            hipLaunchKernelGGL(coord_absmax_kernel, dim3(1), dim3(kShiftThreads), 0, c->stream, c->n,
                               (const int *)c->d_flags, (const double *)c->d_x, (const double *)c->d_y,
                               (const double *)c->d_z, c->d_delta.get());  // (d_delta has been consumed by the launch above)
            double truth = INFINITY;
            HIPCHK(hipMemcpyAsync(&truth, c->d_delta, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            c->stage_used = 0;  // (the ring's copies have completed)
            bound = truth;
        }
        c->coord_max = bound;
        if ((c->coord_max > kScreen32MaxCoord) != was64) ++c->config_rev;
    }
    c->staged_copies = true;  // coordinates reached the device outside the MoveList ...
    c->main_writes = true;    // ... on the main stream: the side stream waits for the event behind them
    c->dirty_atoms.clear();   // (apply_box() set all_dirty)
    for (SweepView &v : c->view) v.A_valid = v.C_valid = false;
    c->view[1].pos_valid = false;  // (view 0's packed positions were shifted by the same launch)
    c->rank_used_valid = false;
    c->rank_saved.clear();
    c->perm_ranked = false;
    c->have_polar_result = false;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Grand-canonical moves without a re-upload.  The engine's atom order is its own business (sums are
// over all atoms / pairs), so an inserted molecule takes the slots a removed one of the same size
// left, or new slots at the end, and a removed molecule leaves holes; both then look like a "moved"
// set of atoms to the incremental machinery (coefficient entries, pair / field / LRC tile partials).
// Return value 1 = not possible incrementally (context full, molecule too large, a solver mode that
// keeps ordered data): the caller uploads the whole configuration again.
// ---------------------------------------------------------------------------------------------
static bool gs_order_mode(const mpmc_hip_ctx *c) {  // Gauss-Seidel on the chain kernel: the view order is the caller's
    const mpmc_hip_params &P = c->par;
    return !P.rd_only && P.polarization && !P.polar_zodid && (P.polar_gs || P.polar_gs_ranked) && c->opt.pair_coef != 0 &&
           c->opt.persistent_gs != 0 && !c->exact_polar;  // (the exact dipoles ignore the solver flags)
}

// dense: the caller brings the per-atom data of the dense modes (mpmc_hip_edit_molecules).  insert_molecule() and
// remove_molecule() cannot, and answer 1 in those modes.
static bool edits_supported(const mpmc_hip_ctx *c, bool dense = false) {
    const mpmc_hip_params &P = c->par;
    if (!c->have_atoms || c->all_dirty || !c->opt.incremental || !c->opt.incremental_pairs || !c->opt.pair_coef) return false;
    if (!dense) {
        if (c->disp_on) return false;  // disp_expansion: c6 / c8 / c10 of the new atoms are missing (the caller uploads again)
        if (c->at_on) return false;    // axilrod_teller: c9 is
        if (c->rdc_order) return false;  // rd_crystal and set_rd_form: pinned to the same answer
        if (c->rd_form) return false;
    }
    if (c->vdw_on) return false;     // polarvdw: the coupled-dipole matrix is not patched by edits
    if (c->exact_polar) return false;  // exact dipoles: the expanded matrix is not patched by edits (as on its Gauss-Seidel path)
    // Gauss-Seidel: only with the chain kernel, whose view is rebuilt from the order the caller states afterwards
    if (!P.rd_only && P.polarization && (P.polar_gs || P.polar_gs_ranked) && !gs_order_mode(c)) return false;
    return true;
}

static int launch_edits(mpmc_hip_ctx *c, const EditList &ed) {
    SweepView &v0 = c->view[0];
    EditTargets t;
    t.x = c->d_x;
    t.y = c->d_y;
    t.z = c->d_z;
    t.q = c->d_q;
    t.alpha = c->d_alpha;
    t.eps = c->d_eps;
    t.sig = c->d_sig;
    t.molmass = c->d_molmass;
    t.mol = c->d_mol;
    t.flags = c->d_flags;
    t.slot_of_atom = v0.d_slot;
    t.idx_of_slot = v0.d_idx;
    t.px = v0.px;
    t.py = v0.py;
    t.pz = v0.pz;
    t.palpha = v0.palpha;
    t.pflags = v0.pflags;
    t.c6 = c->disp_on ? c->d_c6.get() : nullptr;
    t.c8 = c->disp_on ? c->d_c8.get() : nullptr;
    t.c10 = c->disp_on ? c->d_c10.get() : nullptr;
    t.at_a = c->at_on ? c->d_at_a.get() : nullptr;
    t.at_g = c->at_on ? c->d_at_g.get() : nullptr;
    drop_polar_result(c);  // (mark_edited(): the result of the configuration before the edit cannot be asked for any more)
    if (flush_moves(c)) return -1;  // keep the order of the caller's operations
    c->main_writes = true;
    hipLaunchKernelGGL(apply_edits_kernel, dim3(1), dim3(64), 0, c->stream, ed, t);
    HIPCHK(hipGetLastError());
    return 0;
}

static void mark_edited(mpmc_hip_ctx *c, int first, int count) {
    for (int i = 0; i < count; ++i) {
        c->dirty_atoms.push_back(first + i);
        c->lrc_dirty_atoms.push_back(first + i);
    }
    if ((int)c->dirty_atoms.size() > 4 * kMaxDirty) c->all_dirty = true;
    c->have_polar_result = false;
    c->self_valid = false;
    c->rank_used_valid = false;  // (polar_gs_ranked: the next call sorts the metric on the host)
    c->edited = true;
    ++c->config_rev;
}

extern "C" int mpmc_hip_slot_count(mpmc_hip_ctx *c) { return c ? c->n : 0; }

// What an inserted molecule brings beyond the arguments of insert_molecule(): null outside the mode that reads it.
struct DenseAtomData {
    const double *c6 = nullptr, *c8 = nullptr, *c10 = nullptr;  // disp_expansion
    const double *c9 = nullptr;                                  // axilrod_teller (effective)
};
static int remove_checked(mpmc_hip_ctx *c, int first, int count);
static int insert_checked(mpmc_hip_ctx *c, int count, const double *x, const double *y, const double *z, const double *charge,
                          const double *polarizability, const double *epsilon, const double *sigma, const double *mass,
                          int frozen, const DenseAtomData &dd, int *first_slot);

// (where a molecule goes: place_molecule(), step_plan.h)
// View slots an insertion at `first` appends: a polarizable site takes the atom slot's old view slot if it has one.
static int new_view_slots(const mpmc_hip_ctx *c, int first, int count, const double *polarizability) {
    return count_new_view_slots(c->view[0].slot_of_atom, gs_order_mode(c), first, count, polarizability);
}

extern "C" int mpmc_hip_remove_molecule(mpmc_hip_ctx *c, int first, int count) {
    if (!c || !c->have_atoms) return fail("MPMC_HIP: remove_molecule: no configuration uploaded");
    if (c->in_flight) return fail("MPMC_HIP: remove_molecule between energy_begin() and energy_end()");
    if (first < 0 || count <= 0 || first + count > c->n)
        return fail("MPMC_HIP: remove_molecule: range [%d, %d) outside [0, %d)", first, first + count, c->n);
    for (int i = 0; i < count; ++i)
        if (!c->slot_valid[first + i]) return fail("MPMC_HIP: remove_molecule: slot %d holds no atom", first + i);
    if (count > kMaxEdit || !edits_supported(c)) return 1;
    return remove_checked(c, first, count);
}

// The removal itself, every condition checked by the caller.
static int remove_checked(mpmc_hip_ctx *c, int first, int count) {
    HIPCHK(hipSetDevice(c->device));
    SweepView &v0 = c->view[0];
    EditList ed;
    memset(&ed, 0, sizeof(ed));
    ed.n = count;
    for (int i = 0; i < count; ++i) {
        ed.idx[i] = first + i;
        ed.at_g[i] = 1.0;  // (the pad value of set_axilrod_teller)
        // the view slot stays with the atom slot, as a hole -- except in Gauss-Seidel modes, where the view is rebuilt
        // from the caller's order (mpmc_hip_set_sweep_order) and is not patched here
        ed.vslot[i] = gs_order_mode(c) ? -1 : v0.slot_of_atom[first + i];
        ed.mol[i] = -2 - (first + i);
        ed.flags[i] = 0;
        c->slot_valid[first + i] = 0;
        c->slot_polar[first + i] = 0;
    }
    if (launch_edits(c, ed)) return -1;
    c->holes.push_back(std::make_pair(first, count));
    c->n_valid -= count;
    mark_edited(c, first, count);
    if (gs_order_mode(c)) {
        c->order_stale = true;  // (the view's data are reconciled by set_sweep_order + the next energy())
        v0.pos_valid = false;
    }
    return 0;
}

extern "C" int mpmc_hip_insert_molecule(mpmc_hip_ctx *c, int count, const double *x, const double *y, const double *z,
                                        const double *charge, const double *polarizability, const double *epsilon,
                                        const double *sigma, const double *mass, int frozen, int *first_slot) {
    if (!c || !c->have_atoms) return fail("MPMC_HIP: insert_molecule: no configuration uploaded");
    if (c->in_flight) return fail("MPMC_HIP: insert_molecule between energy_begin() and energy_end()");
    if (count <= 0 || !x || !y || !z || !charge || !polarizability || !epsilon || !sigma || !mass || !first_slot)
        return fail("MPMC_HIP: insert_molecule: bad arguments");
    if (count > kMaxEdit || !edits_supported(c)) return 1;
    HIPCHK(hipSetDevice(c->device));
    note_coords(c, x, y, z, count);
    int first, hole;
    if (!place_molecule(c->holes, c->n, c->max_atoms, count, first, hole)) return 1;
    if (c->view[0].nv + new_view_slots(c, first, count, polarizability) > c->view[0].cap) return 1;
    return insert_checked(c, count, x, y, z, charge, polarizability, epsilon, sigma, mass, frozen, DenseAtomData(), first_slot);
}

// The insertion itself: room in the context and in the view checked by the caller, which has also noted the coordinates.
static int insert_checked(mpmc_hip_ctx *c, int count, const double *x, const double *y, const double *z, const double *charge,
                          const double *polarizability, const double *epsilon, const double *sigma, const double *mass,
                          int frozen, const DenseAtomData &dd, int *first_slot) {
    SweepView &v0 = c->view[0];
    int first, hole;
    place_molecule(c->holes, c->n, c->max_atoms, count, first, hole);
    const bool gs_mode = gs_order_mode(c);
    if (hole >= 0)
        c->holes.erase(c->holes.begin() + hole);
    else {
        c->n += count;
        c->slot_valid.resize(c->n, 0);
        c->slot_polar.resize(c->n, 0);
        v0.slot_of_atom.resize(c->n, -1);
        const int npad = round_up(c->n, 128);
        if (npad != c->npad) {  // the tile grids of the pair / field / LRC partials change shape
            c->npad = npad;
            grid_grew(c);
        }
    }
    double mm = 0.0;
    for (int i = 0; i < count; ++i) mm += mass[i];
    const int mol = c->next_mol++;
    EditList ed;
    memset(&ed, 0, sizeof(ed));
    ed.n = count;
    for (int i = 0; i < count; ++i) {
        const int a = first + i;
        int s = gs_mode ? -1 : v0.slot_of_atom[a];
        if (!gs_mode && polarizability[i] != 0.0 && s < 0) {
            s = v0.nv++;
            v0.slot_of_atom[a] = s;
            v0.h_idx.resize(v0.nv);
            v0.h_idx[s] = a;
        }
        ed.idx[i] = a;
        ed.vslot[i] = s;
        ed.mol[i] = mol;
        ed.flags[i] = kValid | (frozen ? kFrozen : 0);
        ed.x[i] = x[i];
        ed.y[i] = y[i];
        ed.z[i] = z[i];
        ed.q[i] = charge[i];
        ed.alpha[i] = polarizability[i];
        ed.eps[i] = epsilon[i];
        ed.sig[i] = sigma[i];
        ed.molmass[i] = mm;
        if (dd.c6) {
            ed.c6[i] = dd.c6[i];
            ed.c8[i] = dd.c8[i];
            ed.c10[i] = dd.c10[i];
        }
        ed.at_g[i] = 1.0;
        if (dd.c9) at_site_values(polarizability[i], dd.c9[i], ed.at_a[i], ed.at_g[i]);
        c->slot_valid[a] = 1;
        c->slot_polar[a] = (polarizability[i] != 0.0);
    }
    const int nvpad = std::max(128, round_up(v0.nv, 128));
    if (nvpad != v0.nvpad) {
        v0.nvpad = nvpad;
        v0.A_valid = false;
    }
    if (launch_edits(c, ed)) return -1;
    c->n_valid += count;
    mark_edited(c, first, count);
    if (gs_mode) {  // the view is rebuilt from the order the caller states next
        c->order_stale = true;
        v0.pos_valid = false;
    }
    *first_slot = first;
    return 0;
}

// Several removals and insertions in one call, with the per-atom data of the dense modes (mpmc_hip.h).  Two halves: the
// first decides every answer other than 0 on copies of the hole list and the slot count and changes nothing; the second
// is the sequence of remove_checked() / insert_checked() the two old entries would run.
constexpr int kMaxEditMolecules = 8;
extern "C" int mpmc_hip_edit_molecules(mpmc_hip_ctx *c, int nremove, const int *remove_first_slot, const int *remove_count,
                                       int ninsert, const mpmc_hip_molecule *insert, int *insert_first_slot) {
    if (!c || !c->have_atoms) return fail("MPMC_HIP: edit_molecules: no configuration uploaded");
    if (c->in_flight) return fail("MPMC_HIP: edit_molecules between energy_begin() and energy_end()");
    if (nremove < 0 || ninsert < 0 || (nremove > 0 && (!remove_first_slot || !remove_count)) ||
        (ninsert > 0 && (!insert || !insert_first_slot)))
        return fail("MPMC_HIP: edit_molecules: bad arguments");
    if (nremove > kMaxEditMolecules || ninsert > kMaxEditMolecules) return 1;
    // ---- errors
    std::vector<char> leaving(c->n, 0);
    size_t atoms = 0;
    bool too_large = false;
    for (int r = 0; r < nremove; ++r) {
        const int first = remove_first_slot[r], count = remove_count[r];
        if (first < 0 || count <= 0 || count > c->n || first > c->n - count)
            return fail("MPMC_HIP: edit_molecules: removal %d: range [%d, %d + %d) outside [0, %d)", r, first, first, count, c->n);
        for (int i = 0; i < count; ++i) {
            if (!c->slot_valid[first + i] || leaving[first + i])
                return fail("MPMC_HIP: edit_molecules: removal %d: slot %d holds no atom", r, first + i);
            leaving[first + i] = 1;
        }
        too_large = too_large || count > kMaxEdit;
        atoms += count;
    }
    for (int m = 0; m < ninsert; ++m) {
        const mpmc_hip_molecule &M = insert[m];
        if (M.count <= 0 || !M.x || !M.y || !M.z || !M.charge || !M.polarizability || !M.epsilon || !M.sigma || !M.mass)
            return fail("MPMC_HIP: edit_molecules: insertion %d: bad arguments", m);
        if (c->disp_on && (!M.c6 || !M.c8 || !M.c10))
            return fail("MPMC_HIP: edit_molecules: c6 / c8 / c10 missing while disp_expansion is on (insertion %d)", m);
        if (c->at_on && !M.c9) return fail("MPMC_HIP: edit_molecules: c9 missing while axilrod_teller is on (insertion %d)", m);
        too_large = too_large || M.count > kMaxEdit;
        if (M.count > kMaxEdit) continue;
        if (c->at_on)
            for (int i = 0; i < M.count; ++i)
                if (M.polarizability[i] < 0.0)
                    return fail("MPMC_HIP: edit_molecules: negative polarizability %g under axilrod_teller (insertion %d, atom %d)",
                                M.polarizability[i], m, i);
        atoms += M.count;
    }
    // ---- "upload again"
    if (too_large || !edits_supported(c, true)) return 1;
    // (more dirty atoms than the incremental passes list would set all_dirty half way, where the old entries start answering 1)
    if (c->dirty_atoms.size() + atoms > 4 * (size_t)kMaxDirty) return 1;
    {
        std::vector<std::pair<int, int>> holes = c->holes;
        int n = c->n, new_view = 0;
        for (int r = 0; r < nremove; ++r) holes.push_back(std::make_pair(remove_first_slot[r], remove_count[r]));
        for (int m = 0; m < ninsert; ++m) {
            int first, hole;
            if (!place_molecule(holes, n, c->max_atoms, insert[m].count, first, hole)) return 1;
            if (hole >= 0)
                holes.erase(holes.begin() + hole);
            else
                n += insert[m].count;
            new_view += new_view_slots(c, first, insert[m].count, insert[m].polarizability);
        }
        if (c->view[0].nv + new_view > c->view[0].cap) return 1;
    }
    // ---- the edits
    HIPCHK(hipSetDevice(c->device));
    for (int r = 0; r < nremove; ++r)
        if (remove_checked(c, remove_first_slot[r], remove_count[r])) return -1;
    for (int m = 0; m < ninsert; ++m) {
        const mpmc_hip_molecule &M = insert[m];
        note_coords(c, M.x, M.y, M.z, M.count);
        for (int i = 0; i < M.count; ++i)
            if (M.sigma[i] < 0.0) c->negative_sigma = true;  // (as an upload that holds one: Waldman-Hagler is then refused)
        DenseAtomData dd;
        if (c->disp_on) {
            dd.c6 = M.c6;
            dd.c8 = M.c8;
            dd.c10 = M.c10;
        }
        if (c->at_on) dd.c9 = M.c9;
        if (insert_checked(c, M.count, M.x, M.y, M.z, M.charge, M.polarizability, M.epsilon, M.sigma, M.mass, M.frozen, dd,
                           &insert_first_slot[m]))
            return -1;
    }
    return 0;
}

// Gauss-Seidel modes after insert / remove: the polarizable sites in the CALLER's atom order (the order of the
// reference's atom_array, which thole_iterative.c walks and update_ranking() stably re-sorts), as device slots.
// Ignored (0) in the other solver modes, whose result does not depend on an order.
extern "C" int mpmc_hip_set_sweep_order(mpmc_hip_ctx *c, int count, const int *slots) {
    if (!c || !c->have_atoms) return fail("MPMC_HIP: set_sweep_order: no configuration uploaded");
    if (c->in_flight) return fail("MPMC_HIP: set_sweep_order between energy_begin() and energy_end()");
    if (!gs_order_mode(c)) return 0;
    SweepView &v0 = c->view[0];
    if (count < 0 || count > v0.cap || (count > 0 && !slots)) return fail("MPMC_HIP: set_sweep_order: bad arguments");
    std::vector<char> seen(c->n, 0);
    for (int k = 0; k < count; ++k) {
        const int a = slots[k];
        if (a < 0 || a >= c->n || !c->slot_valid[a] || seen[a])
            return fail("MPMC_HIP: set_sweep_order: entry %d (slot %d) is not a distinct atom of the configuration", k, a);
        if (!c->slot_polar[a])
            return fail("MPMC_HIP: set_sweep_order: entry %d (slot %d) is not a polarizable site", k, a);
        seen[a] = 1;
    }
    {   // ... and EVERY polarizable site: a Gauss-Seidel sweep over a subset is a different (silently wrong) energy
        int npolar = 0;
        for (int a = 0; a < c->n; ++a) npolar += (c->slot_valid[a] && c->slot_polar[a]);
        if (count != npolar)
            return fail("MPMC_HIP: set_sweep_order: %d slots stated, the configuration has %d polarizable sites", count, npolar);
    }
    HIPCHK(hipSetDevice(c->device));
    drop_polar_result(c);
    if (flush_moves(c)) return -1;  // queued moves were addressed through the old view
    c->main_writes = true;          // (the slot map below; and a flushed move is a main-stream write the side stream has not seen)
    // how far the new order agrees with the old one: the blocks in front of the first difference keep their data
    int p0 = 0;
    {
        const int m = std::min((int)v0.h_idx.size(), count);
        while (p0 < m && v0.h_idx[p0] == slots[p0]) ++p0;
    }
    const bool keep_prefix = v0.C_valid && v0.rebuild_from < 0 && v0.M_epoch == v0.C_epoch && v0.M_call == c->energy_calls;
    v0.h_idx.assign(slots, slots + count);
    v0.nv = count;
    v0.nvpad = std::max(128, round_up(count, 128));
    v0.slot_of_atom.assign(c->n, -1);
    // staged in pinned memory of their own (the ranked view's staging buffers may still be in flight), copied in
    // stream order: nothing here waits for the device
    if (!c->h_order) {
        HIPCHK(c->h_order.alloc(2 * (size_t)c->max_npad));
    } else {
        HIPCHK(hipEventSynchronize(c->ev_order));  // the previous use of the staging buffer has been copied
    }
    int *h_idx = c->h_order, *h_slot = c->h_order + c->max_npad;
    for (int k = 0; k < c->max_npad; ++k) h_slot[k] = -1;
    for (int k = 0; k < count; ++k) {
        v0.slot_of_atom[slots[k]] = k;
        h_slot[slots[k]] = k;
        h_idx[k] = slots[k];
    }
    HIPCHK(hipMemcpyAsync(v0.d_slot, h_slot, (size_t)c->max_npad * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (count > 0) HIPCHK(hipMemcpyAsync(v0.d_idx, h_idx, count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_order, c->stream));
    v0.pos_valid = false;
    if (keep_prefix) {
        v0.rebuild_from = p0 / 64;  // (C stays "valid": setup_view rebuilds the tail and updates moved atoms' entries)
        v0.C_valid = true;
    } else {
        v0.rebuild_from = -1;
        v0.C_valid = false;
    }
    v0.A_valid = false;
    c->view[1].C_valid = c->view[1].A_valid = false;
    c->rank_used_valid = false;
    c->order_stale = false;
    c->have_polar_result = false;
    ++c->config_rev;
    return 0;
}

// k-vector list in the reference's loop order (coulombic.c:56-70)
static int build_kvectors(mpmc_hip_ctx *c) {
    const int kmax = c->par.ewald_kmax;
    std::vector<KVec> kv;
    const double alpha = c->ewald_alpha;
    for (int l0 = 0; l0 <= kmax; l0++)
        for (int l1 = (!l0 ? 0 : -kmax); l1 <= kmax; l1++)
            for (int l2 = ((!l0 && !l1) ? 1 : -kmax); l2 <= kmax; l2++) {
                if (l0 * l0 + l1 * l1 + l2 * l2 > kmax * kmax) continue;
                const int l[3] = {l0, l1, l2};
                double k[3];
                for (int p = 0; p < 3; p++) {
                    k[p] = 0;
                    for (int q = 0; q < 3; q++) k[p] += 2.0 * kPI * c->recip[p][q] * l[q];
                }
                const double k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
                KVec v;
                v.kx = k[0];
                v.ky = k[1];
                v.kz = k[2];
                v.w = std::exp(-k2 / (4.0 * alpha * alpha)) / k2;
                kv.push_back(v);
            }
    c->d_kvec.reset();
    c->nk = (int)kv.size();
    if (c->nk > 0) {
        HIPCHK(c->d_kvec.alloc(kv.size()));
        HIPCHK(hipMemcpy(c->d_kvec, kv.data(), kv.size() * sizeof(KVec), hipMemcpyHostToDevice));
    }
    c->kvec_valid = true;
    c->recip_part_valid = false;
    return 0;
}

// k list of the Ewald static field: same hemisphere as coulombic_reciprocal, weights with polar_ewald_alpha
static int build_field_kvectors(mpmc_hip_ctx *c) {
    const int kmax = c->par.ewald_kmax;
    const double ea = c->polar_ewald_alpha;
    if (c->d_kvecf && c->kvecf_alpha == ea && c->kvecf_kmax == kmax && c->kvecf_valid) return 0;
    std::vector<KVecF> kv;
    for (int l0 = 0; l0 <= kmax; l0++)
        for (int l1 = (!l0 ? 0 : -kmax); l1 <= kmax; l1++)
            for (int l2 = ((!l0 && !l1) ? 1 : -kmax); l2 <= kmax; l2++) {
                if (l0 * l0 + l1 * l1 + l2 * l2 > kmax * kmax) continue;
                const int l[3] = {l0, l1, l2};
                double k[3];
                for (int p = 0; p < 3; p++) {
                    k[p] = 0;
                    for (int q = 0; q < 3; q++) k[p] += 2.0 * kPI * c->recip[p][q] * l[q];
                }
                const double k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
                KVecF v;
                v.kx = k[0];
                v.ky = k[1];
                v.kz = k[2];
                v.w = std::exp(-k2 / (4.0 * ea * ea)) / k2;
                kv.push_back(v);
            }
    c->d_kvecf.reset();
    c->d_sf.reset();
    c->nkf = (int)kv.size();
    if (c->nkf > 0) {
        HIPCHK(c->d_kvecf.alloc(kv.size()));
        HIPCHK(c->d_sf.alloc(kv.size()));
        HIPCHK(hipMemcpy(c->d_kvecf, kv.data(), kv.size() * sizeof(KVecF), hipMemcpyHostToDevice));
    }
    c->kvecf_alpha = ea;
    c->kvecf_kmax = kmax;
    c->kvecf_valid = true;
    return 0;
}

static int ensure_sym_scratch(SweepView &v) {
    const size_t ncol = 3 * (size_t)v.nvpad;
    const size_t need = ncol * (v.nvpad / kSymChunkAtoms + v.nvpad / kSymRowAtoms);
    if (v.Srow.size() < need) HIPCHK(v.Srow.alloc(need));
    v.Zcol = v.Srow + ncol * (v.nvpad / kSymChunkAtoms);
    return 0;
}

// partial-sum buffers of the tiled coefficient sweep: Srow[nt][192 nt], Zcol[nt][192 nt]
static int ensure_coef_scratch(SweepView &v, int nt) {
    const size_t ncol = 3 * (size_t)kCoefTile * nt;
    // sized for every tile the view can grow to: a grand-canonical insertion that starts a new 64-atom block must not
    // pay a free + re-allocation (a millisecond, with the device idle) in the middle of an energy() call
    const size_t ntcap = (size_t)std::max(nt, v.ntld);
    const size_t need = 4 * (3 * (size_t)kCoefTile * ntcap) * ntcap;  // (two planes: whole-tile or half-tile workgroups)
    if (v.Srow.size() < need) HIPCHK(v.Srow.alloc(need));
    v.Zcol = v.Srow + ncol * nt;
    return 0;
}

static int ensure_view_coef(mpmc_hip_ctx *c, SweepView &v, int nt, hipStream_t st) {
    (void)c;
    // sized for every tile the view can grow to (insert_molecule appends to the view), so the tile stride
    // never changes; tiles start out as zeros (= "no pair"), which is what unused slots must read as
    const int ntld = std::max(nt, (v.cap + kCoefTile - 1) / kCoefTile);
    const size_t need = (size_t)ntld * ntld * kCoefTile * kCoefTile;
    if (v.C.size() < need || v.ntld != ntld) {
        HIPCHK(v.C.alloc(need));
        // on the stream that builds the view (the non-blocking streams do not order themselves after the null stream; and
        // a ranked view may be built on the side stream while the main one is busy: a memset queued THERE would come last)
        HIPCHK(hipMemsetAsync(v.C, 0, need * sizeof(double2), st));
        v.ntld = ntld;
        v.C_valid = false;
    }
    return 0;
}

// cached block inverses M_t + neighbour matrices P_t = M_t D T(t,t-1) of the Gauss-Seidel chain, sized for the view's capacity
static int ensure_view_chain(mpmc_hip_ctx *c, SweepView &v, hipStream_t st) {
    if (v.Minv && v.Lnb_lags >= c->opt.gs_lags) return 0;
    const size_t nbcap = (size_t)(v.cap + 63) / 64;
    for (; v.Lnb_lags < c->opt.gs_lags; ++v.Lnb_lags) {
        HIPCHK(v.Lnb[v.Lnb_lags].alloc(nbcap * kPnbDoubles));
        v.M_epoch = 0;
    }
    if (v.Minv) return 0;
    HIPCHK(v.Minv.alloc(nbcap * kMinvDoubles));
    // the folded inverse has 32 padding lanes per block that no build writes: they must read as zero
    HIPCHK(hipMemsetAsync(v.Minv, 0, nbcap * kMinvDoubles * sizeof(double), st));
    v.M_epoch = 0;
    return 0;
}

static int ensure_view_matrix(SweepView &v) {
    const size_t need = (size_t)(3 * (size_t)v.nvpad) * (3 * (size_t)v.nvpad);
    if (v.A.size() < need) HIPCHK(v.A.alloc(need));
    return 0;
}

// E_static in atom order for every atom: the solver only reduces the partials of the polarizable atoms
// (into its view); the full vector is made when a download or the ranked view needs it
static int ensure_static_field(mpmc_hip_ctx *c) {
    if (!c->es_stale) return 0;
    hipLaunchKernelGGL(field_reduce_kernel, dim3(c->npad / 64), dim3(64 * kFieldGroups), 0, c->stream, c->d_fieldpart,
                       c->es_slots, c->npad, c->d_es);
    c->es_stale = false;
    return 0;
}

// ---- resident Jacobi solver (kernels_resident.h)
template <int K>
constexpr int resident_lds_bytes() {
    return (int)std::max(sizeof(ResidentLds<K>), (size_t)kResFinisherLds);
}
constexpr int kResMaxK = 1;
constexpr int kResidentLdsOnePerCu = 84 * 1024;  // more than half a CU's LDS: at most one workgroup per CU
constexpr int kResidentLdsMax = std::max(kResidentLdsOnePerCu, resident_lds_bytes<kResMaxK>());
static_assert(kResidentLdsMax <= 160 * 1024, "LDS of a CU");
typedef void (*ResidentKernel)(ResidentSolve);
static ResidentKernel resident_kernel_of(int ortho, int K, bool fold) {
    (void)K;  // one tile per tile workgroup is the only geometry in use (see resident_plan)
    if (fold) return ortho ? jacobi_folded_kernel<1> : jacobi_folded_kernel<0>;
    return ortho ? jacobi_resident_kernel<1, 1> : jacobi_resident_kernel<0, 1>;
}
static std::vector<const void *> resident_kernels() {
    std::vector<const void *> v;
    for (int o = 0; o < 2; ++o) {
        for (int K = 1; K <= kResMaxK; ++K) v.push_back(reinterpret_cast<const void *>(resident_kernel_of(o, K, false)));
        v.push_back(reinterpret_cast<const void *>(resident_kernel_of(o, 1, true)));
    }
    return v;
}

// How a solve of nt blocks is spread over the chip: K tiles per tile workgroup, ngroups of them (+ nt finishers), one
// or two workgroups per CU -- whichever leaves the fewest tiles per CU (each tile is one wave's work per SIMD and
// sweep).  ok = false: does not fit (or is not a fixed-count Jacobi-type solve): the multi-launch path runs.
struct ResidentPlan {
    bool ok = false;
    bool fold = false;  // no finisher workgroups: every tile workgroup finishes its two blocks (jacobi_folded_kernel)
    int K = 0, ngroups = 0, lds = 0, nt = 0, ntiles = 0;
};
static ResidentPlan resident_plan(const mpmc_hip_ctx *c, const SweepView &v) {
    ResidentPlan r;
    const mpmc_hip_params &P = c->par;
    if (!c->opt.resident || c->resident_off || c->force_multi_launch || !c->opt.pair_coef || !v.C_valid) return r;
    if (P.polar_zodid || P.polar_gs || P.polar_gs_ranked || P.polar_precision != 0.0) return r;
    if (P.polar_max_iter < 1 || P.polar_max_iter > kResMaxSweeps) return r;
    if (c->device < 64 && g_ctx_on_device[c->device].load() > 1) return r;  // co-residency needs the device to itself
    const int nt = std::max(1, (v.nv + kCoefTile - 1) / kCoefTile);
    if (nt > kResMaxBlocks) return r;
    const int ntiles = nt * (nt + 1) / 2, cus = c->num_cus;
    // One workgroup per CU, one tile per tile workgroup: views of up to 21 blocks (1 344 polarizable sites).  Larger
    // views were tried with 2-5 tiles per workgroup (kernel template parameter K) and with two workgroups per CU: the
    // coefficient set of the 4096-atom boxes fits the register files only with one wave per SIMD or with spills, the
    // product phase then takes 2 us per tile instead of 1.25, and the LJ / Ewald stream no longer overlaps -- slower than
    // the multi-launch path there.
    if (ntiles + nt > cus) return r;
    const int bestK = 1;
    r.ok = true;
    r.K = bestK;
    r.nt = nt;
    r.ntiles = ntiles;
    r.ngroups = ntiles;
    r.fold = nt <= std::min(c->opt.res_fold, kFoldMaxBlocks);
    const int need = resident_lds_bytes<1>();
    const bool one = true;
    r.lds = one ? std::max(need, kResidentLdsOnePerCu) : need;
    return r;
}

static int ensure_view_resident(mpmc_hip_ctx *c, SweepView &v) {
    const int pld = std::min(std::max(1, v.ntld), kResMaxBlocks);
    const size_t pstride = (size_t)pld * pld * 384;
    if (!v.resP || v.res_pld != pld) {
        HIPCHK(v.resP.alloc(3 * pstride));  // (two parities; three rotating buffers when folded)
        v.res_pld = pld;
        v.resP_armed = false;
    }
    if (!v.resP_armed) {
        // both 32-bit halves of the sentinel are the same word
        static_assert((kGsSentinel >> 32) == (kGsSentinel & 0xffffffffull), "sentinel halves");
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)v.resP, (int)(kGsSentinel & 0xffffffffull), 3 * pstride * 2, c->stream));
        v.resP_armed = true;
    }
    if (!v.respub) HIPCHK(v.respub.alloc((size_t)kResMaxSweeps * 3 * v.cap));
    return 0;
}

#include "engine_polar.inc"

// the 16-double result record goes straight into mapped pinned host memory (no copy engine / copy kernel)
// followed by a sequence number the host spins on (no dependence on the device's sync-scheduling mode)
__global__ __launch_bounds__(mpmc::kReduceThreads) void publish_result_kernel(
    double *__restrict__ d_res, volatile double *__restrict__ h_res, int n, double seq,
    const double *__restrict__ energy_part, int nt, int n_total, const unsigned *__restrict__ gs_err0,
    const unsigned *__restrict__ gs_err1, const double *__restrict__ recip_chunk, int nrecip, unsigned zero_mask,
    const double *__restrict__ pair_part, int pair_rows, int pair_slot, unsigned skip_mask) {
    // (skip_mask: slots the side stream publishes itself -- publish_side_kernel -- and this kernel neither reads nor writes)
    // ---- the LJ / real-space Ewald tile partials (reduce_rows_kernel's arithmetic in reduce_rows_kernel's order: this
    // used to be a launch of its own behind the pair kernel): thread t takes rows t, t + 1024, ..., 64-lane butterflies,
    // then the 16 wave sums in order
    if (pair_rows > 0) {
        __shared__ double s[mpmc::kReduceThreads / 64][4];
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = threadIdx.x; r < pair_rows; r += mpmc::kReduceThreads) {
            const double *p = pair_part + (size_t)r * mpmc::kPairChannels;
#pragma unroll
            for (int c = 0; c < mpmc::kPairChannels; ++c) acc[c] += p[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc[c] = mpmc::wave_sum(acc[c]);
            if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6][c] = acc[c];
        }
        __syncthreads();
        if ((int)threadIdx.x < mpmc::kPairChannels) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < mpmc::kReduceThreads / 64; ++w) t += s[w][threadIdx.x];
            d_res[pair_slot + threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x >= 64) return;  // the record itself is one wave's work
    // terms this call does not compute (no long-range correction, Wolf instead of Ewald, no polarization) are zero
    const bool mine = (int)threadIdx.x < n && !((skip_mask >> threadIdx.x) & 1u);
    if (mine && ((zero_mask >> threadIdx.x) & 1u)) d_res[threadIdx.x] = 0.0;
    double rec = 0.0, e = 0.0, r = 0.0;
    if (nrecip > 0) {  // reciprocal-space sum: chunk sums in chunk order
        for (int t = threadIdx.x; t < nrecip; t += 64) rec += recip_chunk[t];
        rec = mpmc::wave_sum(rec);
    }
    if (nt > 0) {
        // U_pol and <rrms> from the per-block sums the finish step left (fixed order)
        for (int t = threadIdx.x; t < nt; t += 64) {
            e += energy_part[2 * t];
            r += energy_part[2 * t + 1];
        }
        e = mpmc::wave_sum(e);
        r = mpmc::wave_sum(r);
    }
    // the record: what the other kernels left in d_res, with this kernel's sums in their slots (one wave: the values
    // travel in registers, a lane's own earlier store to its slot is ordered before its load)
    double v = 0.0;
    if (mine) {
        v = d_res[threadIdx.x];
        if ((zero_mask >> threadIdx.x) & 1u) v = 0.0;
        if (nrecip > 0 && threadIdx.x == R_RECIP) v = rec;
        // error words of the persistent launches of this call travel with the result record
        if (threadIdx.x == R_GS_ERR) v = ((gs_err0 && *gs_err0) ? 1.0 : 0.0) + ((gs_err1 && *gs_err1) ? 2.0 : 0.0);
        if (nt > 0 && threadIdx.x == R_UPOL) v = -0.5 * e;
        if (nt > 0 && threadIdx.x == R_RRMS) v = r / (double)n_total;  // mean over ALL atoms (polar.c:21-27)
        d_res[threadIdx.x] = v;
        h_res[threadIdx.x] = v;
    }
    __threadfence_system();
    if (threadIdx.x == 0) h_res[n] = seq;
}

// The side stream's part of the record (the LJ / Ewald slots of side_mask), published by the side stream itself behind
// its last kernel: the main stream then needs no join event in front of its own publish launch (a cross-stream wait
// cost the S-POL(1024) step ~8 us), and mpmc_hip_energy_end() waits for both sequence numbers.  Same arithmetic as
// publish_result_kernel for these slots (zeros for terms the call does not compute; chunk sums in chunk order).
__global__ __launch_bounds__(64) void publish_side_kernel(double *__restrict__ d_res, volatile double *__restrict__ h_res2,
                                                            int n, double seq, const double *__restrict__ recip_chunk,
                                                            int nrecip, unsigned zero_mask, unsigned side_mask) {
    double rec = 0.0;
    if (nrecip > 0) {
        for (int t = threadIdx.x; t < nrecip; t += 64) rec += recip_chunk[t];
        rec = mpmc::wave_sum(rec);
    }
    if ((int)threadIdx.x < n && ((side_mask >> threadIdx.x) & 1u)) {
        double v = d_res[threadIdx.x];
        if ((zero_mask >> threadIdx.x) & 1u) v = 0.0;
        if (nrecip > 0 && threadIdx.x == R_RECIP) v = rec;
        d_res[threadIdx.x] = v;
        h_res2[threadIdx.x] = v;
    }
    __threadfence_system();
    if (threadIdx.x == 0) h_res2[n] = seq;
}
constexpr unsigned kSideSlots = (1u << R_RD_PAIR) | (1u << R_ES_REAL) | (1u << R_ES_INTRA) | (1u << 3) | (1u << R_LRC) |
                                (1u << R_RECIP) | (1u << R_SELF) | (1u << R_DISP) | (1u << R_DISP_LRC) | (1u << R_AT) |
                                (1u << R_RDC_SELF);

// LJ / real-space Ewald tile kernel (graph slot GS_PAIR).  Tile partials persist: after a single-molecule
// move only the tiles of the moved atoms' blocks are recomputed.
static int launch_pair_kernel(mpmc_hip_ctx *c, const DevAtoms &a, const DevBox &bx, hipStream_t sb,
                              bool with_recip = false) {
    const mpmc_hip_params &P = c->par;
    const int ntile = c->npad / 64;
    PairParams pp;
    pp.ewald_alpha = c->ewald_alpha;
    pp.temperature = P.temperature;
    pp.rd_only = P.rd_only;
    pp.fh_order = P.feynman_hibbs ? P.feynman_hibbs_order : 0;
    pp.wolf = P.wolf;
    pp.erfaRoverR = std::erf(c->ewald_alpha * c->cutoff) / c->cutoff;
    DirtyBlocks sel = c->call.dirty_blocks;
    if (!c->pair_part_valid) sel.n = 0;
    const dim3 grid(ntile, sel.n > 0 ? sel.n : ntile), block(64 * kPairWaves);
    c->call.recip_fused = false;
    if (c->pair_part_valid && c->dirty_atoms.empty()) return 0;  // nothing moved since the partials were made
    // the step's move, when this launch carries it (steps without polarization: enqueue_direct)
    MoveList mv;
    mv.n = 0;
    MoveTargets mt = {c->d_x, c->d_y, c->d_z, c->view[0].d_slot, c->view[0].px, c->view[0].py, c->view[0].pz};
    if (c->call.moves_in_pair && c->pending.n > 0) {
        mv = c->pending;
        c->pending.n = 0;
    } else if (c->call.side_carry && sb == c->stream2 && c->call.side_moves.n > 0) {
        // A steady-state polarizable step: the main stream applies the move inside its coefficient update
        // (update_coef_moves_kernel) and this launch -- the first of the side stream that reads coordinates -- applies the
        // SAME move for itself: no thread of either kernel reads a moved atom's position from memory, both write the same
        // bits into the coordinate arrays, and each stream's later kernels come behind their own stream's writer.  So the
        // two streams need no fork event (recording one costs the main stream ~5 us between its first two launches).
        mv = c->call.side_moves;
    }
    c->call.side_moves.n = 0;
    c->call.moves_in_pair = false;
    c->call.pair_moves = mv;
    // cavity_autoreject_absolute: the close-contact count of the same tiles, into the channel the pair kernel has cleared
    auto contacts = [&] {
        if (c->autoreject_scale == 0.0) return;
        hipLaunchKernelGGL(contact_tile_kernel, grid, dim3(64 * kContactWaves), 0, sb, a, bx, c->autoreject_scale, sel,
                           c->d_pairpart, kPairChannels, (int)R_CONTACTS, mv);
    };
    if (with_recip && c->opt.fuse_recip && c->call.plain_launches && c->nk > 0 &&
        (c->nk + 63) / 64 <= ntile) {
        // the reciprocal-space partials of the same blocks ride in a second z-slice of this launch (pair_recip_kernel) when
        // both passes are of the same kind: incremental over the same dirty blocks, or full
        DirtyBlocks rsel = c->call.dirty_blocks;
        if (!c->recip_part_valid || !c->call.pair_part_valid_before) rsel.n = 0;
        const bool recip_skipped = c->recip_part_valid && c->call.pair_part_valid_before && c->dirty_atoms.empty();
        if (!recip_skipped && rsel.n == sel.n) {
            const dim3 g2(grid.x, grid.y, 2);
            RecipJob rj = {(const KVec *)c->d_kvec, c->nk, c->d_sfpart};
            if (pp.fh_order == 0)
                hipLaunchKernelGGL(pair_recip_kernel<0>, g2, block, 0, sb, a, bx, pp, sel, c->d_pairpart, mv, mt, rj);
            else if (pp.fh_order == 2)
                hipLaunchKernelGGL(pair_recip_kernel<2>, g2, block, 0, sb, a, bx, pp, sel, c->d_pairpart, mv, mt, rj);
            else
                hipLaunchKernelGGL(pair_recip_kernel<4>, g2, block, 0, sb, a, bx, pp, sel, c->d_pairpart, mv, mt, rj);
            HIPCHK(hipGetLastError());
            contacts();
            c->pair_part_valid = true;
            c->recip_part_valid = true;
            c->call.recip_fused = true;
            return 0;
        }
    }
    if (pp.fh_order == 0)
        HIPCHK(launch_slot(c, GS_PAIR, pair_rd_es_kernel<0>, grid, block, sb, a, bx, pp, sel, c->d_pairpart, mv, mt));
    else if (pp.fh_order == 2)
        HIPCHK(launch_slot(c, GS_PAIR, pair_rd_es_kernel<2>, grid, block, sb, a, bx, pp, sel, c->d_pairpart, mv, mt));
    else
        HIPCHK(launch_slot(c, GS_PAIR, pair_rd_es_kernel<4>, grid, block, sb, a, bx, pp, sel, c->d_pairpart, mv, mt));
    contacts();
    c->pair_part_valid = true;
    return 0;
}

// partial structure factors of the moved atoms' blocks (graph slot GS_RECIP), or of all blocks
static int launch_recip_partial(mpmc_hip_ctx *c, const DevAtoms &a, hipStream_t sb) {
    const int ntile = c->npad / 64;
    DirtyBlocks rsel = c->call.dirty_blocks;
    if (!c->recip_part_valid || !c->call.pair_part_valid_before) rsel.n = 0;
    if (c->recip_part_valid && c->call.pair_part_valid_before && c->dirty_atoms.empty()) return 0;  // nothing moved
    HIPCHK(launch_slot(c, GS_RECIP, recip_partial_kernel, dim3((c->nk + 63) / 64, rsel.n > 0 ? rsel.n : ntile),
                       dim3(64 * kRecipWaves), sb, a, (const KVec *)c->d_kvec, c->nk, rsel, c->d_sfpart));
    c->recip_part_valid = true;
    return 0;
}

#include "engine_dense.inc"

static int launch_publish(mpmc_hip_ctx *c) {
    const bool do_polar = c->call.do_polar;
    // (one wave unless the kernel also has the pair kernel's tile partials to add up)
    HIPCHK(launch_slot(c, GS_PUBLISH, publish_result_kernel, dim3(1), dim3(c->call.pair_rows_to_sum > 0 ? kReduceThreads : 64),
                       c->stream, c->d_res, c->h_res_dev,
                       (int)R_COUNT, (double)c->energy_calls, do_polar ? c->energy_part : (const double *)nullptr,
                       do_polar ? c->energy_nt : 0, c->n_valid,
                       c->call.gs_used[0] ? (const unsigned *)(c->view[0].gsflags + 1) : (const unsigned *)nullptr,
                       c->call.gs_used[1] ? (const unsigned *)(c->view[1].gsflags + 1) : (const unsigned *)nullptr,
                       (const double *)c->d_recipsum, c->call.split ? 0 : c->call.recip_chunks, c->call.res_zero_mask,
                       (const double *)c->d_pairpart, c->call.pair_rows_to_sum, (int)R_RD_PAIR, c->call.split ? kSideSlots : 0u));
    return 0;
}

// 64-atom blocks touched by the moves since the last call (n = 0: recompute every tile)
static void collect_dirty_blocks(mpmc_hip_ctx *c) {
    DirtyBlocks &d = c->call.dirty_blocks;
    if (c->all_dirty || !c->opt.incremental_pairs || !blocks_of(c->dirty_atoms, d)) {
        positions_unknown(c);
        memset(&d, 0, sizeof(d));
    }
    c->call.pair_part_valid_before = c->pair_part_valid;  // false whenever the dirty-block list cannot be trusted
}

// The one place an evaluation starts: energy_begin(), and energy_end() when it has to repeat a call.
static void begin_call(mpmc_hip_ctx *c) {
    ++c->energy_calls;
    c->ev_next = 0;
    c->recs.clear();
    c->call = CallState();
    c->psweep.drop();  // nobody asked for the previous call's dipoles: its pending sweeps are never launched
    collect_dirty_blocks(c);
}

// The predicates of the call, from the parameters, the options and what is pending: launches nothing, changes nothing but
// c->call.
static void plan_call(mpmc_hip_ctx *c) {
    const mpmc_hip_params &P = c->par;
    CallState &k = c->call;
    k.do_polar = !P.rd_only && P.polarization;
    k.exact = k.do_polar && c->exact_polar;
    k.gs_mode = (P.polar_gs || P.polar_gs_ranked) && !k.exact;
    // ---- fork: LJ / Ewald kernels (fp64-VALU bound) run on stream2 while the polarization chain
    // (HBM bound) runs on the main stream -- the device-side analogue of the reference starting its
    // polarization worker before the other energy terms (energy.c:108-129, :181-186).
    // (without polarization there is nothing to overlap with: one stream, and no fork / join events -- a cross-stream
    //  dependency costs several microseconds each way, a quarter of an LJ-only step)
    k.two_streams = c->opt.overlap && k.do_polar;
    k.plain_launches = c->graph_mode == GM_DIRECT && !c->opt.graph;  // (neither changes while the call is enqueued)
    const bool do_polar = k.do_polar, two_streams = k.two_streams;
    // A single-molecule move of a steady-state polarizable step is applied inside the coefficient update of view 0
    // (update_coef_moves_kernel) instead of by a launch of its own; setup_view() falls back to the plain way whenever
    // that update does not happen.  (Not in the Gauss-Seidel modes: their ranking kernels read the coordinates first.)
    // (Gauss-Seidel modes, round 3: with the chain kernel's data -- whose maintenance follows the coefficient update
    //  inside setup_view() -- the move rides in update_coef_moves_kernel too, as a launch of its own in front of the block
    //  matrices instead of apply_moves_kernel + update_coef_kernel; the side stream, whose ranking kernels read the
    //  coordinates, applies the same move for itself as before (side_apply).  Option "gs_fuse_moves".)
    k.moves_deferred = c->opt.fuse_moves && c->pending.n > 0 && k.plain_launches && do_polar && !P.polar_zodid && !k.exact &&
                       (!k.gs_mode || (c->opt.gs_fuse_moves && gs_order_mode(c))) && P.polar_precision == 0.0 && c->opt.overlap &&
                       c->opt.pair_coef && !c->all_dirty && c->view[0].C_valid && c->view[0].pos_valid;
    // Without polarization the pair kernel is the first kernel of the step that reads coordinates: the move rides in it.
    // (The long-range-correction and self-term kernels in front of it read parameters only.)
    k.moves_in_pair = !k.moves_deferred && c->opt.fuse_moves && c->pending.n > 0 && k.plain_launches && !do_polar &&
                      !c->dirty_atoms.empty();
    // (the pair kernel is launched whenever an atom moved; the long-range-correction kernels in front of it read
    //  parameters only)
    k.side_carry = k.moves_deferred && !k.gs_mode && c->opt.side_moves && !c->main_writes && !c->dirty_atoms.empty() &&
                   c->pending.n <= kMaxMoves;
    // The side stream publishes its own slots of the record (no join event) in the Jacobi-type modes; the Gauss-Seidel
    // modes keep the join (their ranking kernels share slots and streams with the chain), and so does graph capture.
    k.split = two_streams && c->opt.split_record && !k.gs_mode && k.plain_launches;
    // Enqueue order: the host needs ~3 us per launch and the polarization chain is the critical path, so
    // with a fixed iteration count the chain is enqueued up to its first sweep (by then the device has
    // ~40 us of work queued), then the side-stream kernels, then the remaining sweeps (option "side_after":
    // after 1, 2 and 3 sweeps measured 5 910 / 5 820 / 5 750 steps/s, within box noise); in precision mode
    // the chain synchronises with the host every iteration, so the side stream is fed first.
    k.polar_first = do_polar && two_streams && P.polar_precision == 0.0;
    // Early publication.  A fixed-count Jacobi solve whose last sweep is deferred knows U_pol after the finish of sweep
    // ceil(n / 2) (engine_polar.inc, defer_last_sweep()); sweeps up to n - 1 serve only a later reader of the dipoles.  With
    // the side stream publishing its own slots nothing else of the record is the main stream's, so run_polarization()
    // launches the publish kernel right behind that finish and leaves the remaining sweeps to whoever asks for the
    // dipoles (PendingSweep): the next call's launches queue right behind the record.  Not when the call is
    // timed with events (ev_last marks the end of the chain) nor in a captured step: both keep the placement at the end,
    // and the same bits (tests/test_gpu_early_publish.py holds a timed context against an untimed one).
    k.may_publish_early = k.split && k.polar_first && !is_timed_call(c);
}

// The side stream's launches of the call: the static sums, the pair kernel, the dense terms, reciprocal space and self
// term, and its own part of the record (or the join event).  On the main stream when the call has only one.
static int enqueue_side_stream(mpmc_hip_ctx *c) {
    const mpmc_hip_params &P = c->par;
    CallState &k = c->call;
    const bool two_streams = k.two_streams;
    const DevAtoms a = dev_atoms(c);
    const DevBox bx = dev_box(c);
    const int ntile = c->npad / 64;
    hipStream_t sb = two_streams ? c->stream2 : c->stream;
    // after apply_moves: the new coordinates are in place (unless this stream's pair kernel brings the move itself)
    if (two_streams && !(k.side_carry && k.side_moves.n > 0)) side_wait_for_moves(c, sb);
    // ---- the static sums depend on parameters, the volume and WHICH atoms exist -- not on coordinates: summed once,
    // their tile partials kept, and only the tiles of inserted / removed atoms' blocks redone afterwards.  The list of
    // those atoms is read here, by every static sum of the call (this one, launch_disp / launch_rdc / launch_rdform),
    // and cleared behind the last of them.
    const bool lrc_overflow = !blocks_of(c->lrc_dirty_atoms, k.lrc_blocks);
    k.lrc_edited = !c->lrc_dirty_atoms.empty();
    // ---- LJ long-range correction (lj.c:56-107)
    if (P.rd_lrc) {
        DirtyBlocks lsel;
        const bool stale = lrc_selection(c, !c->lrc.valid || lrc_overflow, lsel);
        if (static_pass(c, c->lrc, stale, ntile * ntile, R_LRC, sb, [&] {
                hipLaunchKernelGGL(lj_lrc_kernel, dim3(ntile, lsel.n > 0 ? lsel.n : ntile), dim3(64 * kLrcWaves), 0, sb, a, bx,
                                   lsel, c->lrc.part);
            }))
            return -1;
    } else {
        k.res_zero_mask |= 1u << R_LRC;  // (zeroed by the publish kernel: a memset is a launch of its own)
        c->lrc.valid = false;
    }

    // ---- fused pair kernel: LJ(+FH) and real-space Ewald(+FH, + intra-molecular screening)
    const bool ewald_recip = !P.rd_only && !P.wolf && c->nk > 0;
    if (ewald_recip) {
        // partial structure factors per 64-atom block stay resident; only the moved blocks are redone
        const size_t need = (size_t)(c->max_npad / 64) * c->nk;
        const size_t nchunk = (c->nk + 63) / 64;
        if (c->d_sfpart.size() < need || c->d_recipsum.size() < nchunk) {
            HIPCHK(c->d_sfpart.alloc(need));
            HIPCHK(c->d_recipsum.alloc(nchunk));
            c->recip_part_valid = false;
        }
    }
    {
        ScopedTimer t(c, T_PAIR, sb);
        if (launch_pair_kernel(c, a, bx, sb, ewald_recip)) return -1;
        if (two_streams) {
            // beside the polarization chain the sum is free on the side stream, and would be 3.5 us of the main one
            hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(kReduceThreads), 0, sb, c->d_pairpart, ntile * ntile,
                               kPairChannels, c->d_res + R_RD_PAIR);
            k.pair_rows_to_sum = 0;
        } else {
            k.pair_rows_to_sum = ntile * ntile;  // summed by the publish kernel (same arithmetic, one launch less)
        }
    }
    // ---- disp_expansion: exp repulsion + damped C6 / C8 / C10 over ALL pairs, and its long-range correction
    if (c->disp_on) {
        if (launch_disp(c, a, bx, sb)) return -1;
        k.res_zero_mask |= 1u << R_RDC_SELF;
    } else if (c->rdc_order) {
        // ---- rd_crystal: Lennard-Jones over the lattice images, its self part and its long-range correction
        if (launch_rdc(c, a, bx, sb)) return -1;
    } else if (c->vdw_on) {
        // ---- polarvdw: repulsion-only Lennard-Jones, then the coupled-dipole term (it owns R_AT and R_RDC_SELF here)
        if (launch_vdw(c, a, bx, sb)) return -1;
    } else if (c->rd_form) {
        // ---- set_rd_form: the dense sum of the form, and the LJ form's long-range correction
        if (launch_rdform(c, a, bx, sb)) return -1;
        k.res_zero_mask |= 1u << R_RDC_SELF;
    } else {
        k.res_zero_mask |= (1u << R_DISP) | (1u << R_DISP_LRC) | (1u << R_RDC_SELF);
    }
    // ---- axilrod_teller: the triple-dipole sum over ALL triples that are not on one molecule
    if (c->at_on) {
        if (launch_at(c, a, bx, sb)) return -1;
    } else if (!c->vdw_on) {
        k.res_zero_mask |= 1u << R_AT;
    }
    c->lrc_dirty_atoms.clear();  // (every static sum of the call has consumed it)

    // ---- reciprocal + self (absent under Wolf summation, coulombic.c:27-28)
    if (!P.rd_only && !P.wolf) {
        ScopedTimer t(c, T_RECIP, sb);
        if (c->nk > 0) {
            if (!k.recip_fused && launch_recip_partial(c, a, sb)) return -1;
            hipLaunchKernelGGL(recip_sum_kernel, dim3((c->nk + 63) / 64), dim3(64 * kRecipGroups), 0, sb, c->d_kvec,
                               c->nk, ntile, c->d_sfpart, c->d_recipsum);
            k.recip_chunks = (c->nk + 63) / 64;
        } else {
            k.res_zero_mask |= 1u << R_RECIP;
        }
        // depends on the charges and alpha only: summed at upload / edit / parameter change, then kept in d_res
        if (!c->self_valid || c->self_alpha != c->ewald_alpha) {
            hipLaunchKernelGGL(ewald_self_kernel, dim3(1), dim3(256), 0, sb, a, c->ewald_alpha, c->d_res + R_SELF);
            c->self_valid = true;
            c->self_alpha = c->ewald_alpha;
        }
    } else {
        k.res_zero_mask |= (1u << R_RECIP) | (1u << R_SELF);
        c->self_valid = false;
    }
    if (k.split)
        hipLaunchKernelGGL(publish_side_kernel, dim3(1), dim3(64), 0, sb, c->d_res, c->h_res2_dev, (int)R_COUNT,
                           (double)c->energy_calls, (const double *)c->d_recipsum, k.recip_chunks, k.res_zero_mask,
                           kSideSlots);
    else if (two_streams)
        hipEventRecord(c->ev_join, sb);
    return 0;
}

static void side_stream_once(mpmc_hip_ctx *c) {
    if (c->call.side_done) return;
    c->call.side_done = true;
    c->call.side_rc = enqueue_side_stream(c);
}
static void feed_side_stream(mpmc_hip_ctx *c) {
    if (c->call.side_open) side_stream_once(c);
}
static void publish_early(mpmc_hip_ctx *c) {
    CallState &k = c->call;
    if (!k.side_open || !k.may_publish_early || k.published || k.build_join_pending) return;
    k.published = true;
    k.publish_rc = launch_publish(c);
}

// One evaluation, launch by launch (also what stream capture records for the step graph): plan, fork, polarization chain
// with the side stream fed from inside it (or in front of it), join, publish.
static int enqueue_direct(mpmc_hip_ctx *c) {
    const mpmc_hip_params &P = c->par;
    CallState &k = c->call;
    plan_call(c);
    const bool do_polar = k.do_polar, two_streams = k.two_streams;
    // ---- the pending move, unless a later launch of the call carries it
    if (!k.moves_deferred && !k.moves_in_pair) {
        if (c->opt.side_moves && !c->main_writes && c->pending.n > 0 && two_streams && k.plain_launches)
            k.side_apply = c->pending;  // (the side stream applies it too: no fork event, see side_wait_for_moves)
        if (flush_moves(c)) return -1;
    } else if (k.moves_deferred && k.gs_mode) {
        if (c->opt.side_moves && !c->main_writes) k.side_apply = c->pending;  // (else: the fork event behind the coefficient job)
    }
    if (is_timed_call(c)) hipEventRecord(c->ev_first, c->stream);
    // ---- fork
    if (two_streams && !k.moves_deferred && k.side_apply.n == 0)
        hipEventRecord(c->ev_fork, c->stream);  // (the side stream's wait is issued when it is fed)
    if (!k.polar_first) side_stream_once(c);
    // ---- polarization (main stream); feed_side_stream() and publish_early() act only inside this window
    int polar_iterations = 0, iter_success = 0;
    if (do_polar) {
        k.side_open = k.polar_first;
        const int rc = run_polarization(c, dev_atoms(c), dev_box(c), &polar_iterations, &iter_success);
        k.side_open = false;
        if (rc || k.publish_rc) return -1;
        if (k.moves_deferred) return fail("MPMC_HIP: internal: a deferred move was not applied");
    } else {
        k.res_zero_mask |= (1u << R_UPOL) | (1u << R_RRMS);
    }
    // the resident A only tracks moves while it is being maintained
    if (!do_polar || P.polar_zodid) c->view[0].A_valid = c->view[0].C_valid = false;
    // ---- the side stream, if the chain did not feed it; join
    side_stream_once(c);
    if (k.side_rc) return -1;
    if (c->pending.n > 0 && flush_moves(c)) return -1;  // (a move no launch of this call carried: cannot happen, but cheap)
    k.moves_in_pair = false;
    if (k.build_join_pending) {  // (a builder launch no chain launch of this call waited for)
        hipStreamWaitEvent(c->stream, c->ev_bjoin, 0);
        k.build_join_pending = false;
    }
    if (two_streams && !k.split) hipStreamWaitEvent(c->stream, c->ev_join, 0);
    const bool timed_call = is_timed_call(c);
    if (timed_call) hipEventRecord(c->ev_last, c->stream);
    if (!k.published && launch_publish(c)) return -1;  // (published: run_polarization() has launched it already)
    k.iterations = polar_iterations;
    k.iter_success = iter_success;
    k.timed = timed_call;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// A steady-state MC step (one molecule displaced, everything resident, fixed iteration count) always
// enqueues the same ~25 kernels; only five of them see new arguments (GraphSlotId).  With option
// "step_graph" such a step is captured once into a HIP graph and afterwards replayed with one launch
// after refreshing those five nodes; anything else (uploads, parameter changes, timed calls,
// Gauss-Seidel / precision-controlled solves, moves that miss the incremental paths) goes launch by
// launch.  Results are bit-identical.  OFF by default -- measured on MI355X / ROCm 7.2 (4096-atom box):
// refreshing the five nodes costs 3 us, but hipGraphLaunch of the two-stream graph costs 60 us of host
// time and the replay finishes later than 22 direct launches (237 vs 152 us per energy()); captured on
// one stream the launch drops to 15 us, but the LJ/Ewald kernels no longer overlap the sweeps (183 us).
// ---------------------------------------------------------------------------------------------
static bool graph_eligible(mpmc_hip_ctx *c) {
    const mpmc_hip_params &P = c->par;
    const SweepView &v = c->view[0];
    if (!c->opt.graph || is_timed_call(c) || !c->opt.incremental || !c->opt.incremental_pairs ||
        !c->opt.pair_coef || c->disp_on || c->at_on || c->rdc_order || c->vdw_on || c->rd_form || c->autoreject_scale != 0.0 ||
        c->exact_polar)
        return false;
    if (P.rd_only || !P.polarization || P.polar_zodid || P.polar_gs || P.polar_gs_ranked || P.polar_precision != 0.0 ||
        P.polar_max_iter <= 0)
        return false;
    if (c->all_dirty || c->staged_copies || c->pending.n <= 0 || c->call.dirty_blocks.n < 1) return false;
    if (!v.C_valid || !v.pos_valid || !c->pair_part_valid || !c->field_part_valid) return false;
    if (P.rd_lrc && !c->lrc.valid) return false;
    if (P.polar_ewald && !c->kvecf_valid) return false;
    bool polarizable_moved = false;
    for (int atom : c->dirty_atoms) polarizable_moved |= (v.slot_of_atom[atom] >= 0);
    if (!polarizable_moved || c->dirty_atoms.size() > (size_t)kMaxDirty) return false;
    return true;
}

static void graph_destroy(mpmc_hip_ctx *c) {
    if (c->sg.exec) hipGraphExecDestroy(c->sg.exec);
    if (c->sg.graph) hipGraphDestroy(c->sg.graph);
    c->sg = StepGraph();
}

// after a capture: instantiate and find the five nodes that get new arguments every step
static bool graph_finish_capture(mpmc_hip_ctx *c, hipGraph_t graph) {
    StepGraph &g = c->sg;
    g.graph = graph;
    if (hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0) != hipSuccess) return false;
    size_t nn = 0;
    if (hipGraphGetNodes(g.graph, nullptr, &nn) != hipSuccess || nn == 0) return false;
    std::vector<hipGraphNode_t> nodes(nn);
    if (hipGraphGetNodes(g.graph, nodes.data(), &nn) != hipSuccess) return false;
    int found[GS_NSLOT] = {0, 0, 0, 0, 0, 0};
    for (hipGraphNode_t nd : nodes) {
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nd, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
        hipKernelNodeParams p;
        if (hipGraphKernelNodeGetParams(nd, &p) != hipSuccess) return false;
        for (int s = 0; s < GS_NSLOT; ++s)
            if (g.func[s] && p.func == g.func[s]) {
                g.node[s] = nd;
                found[s]++;
            }
    }
    for (int s = 0; s < GS_NSLOT; ++s)
        if (g.func[s] ? found[s] != 1 : found[s] != 0) return false;  // (a slot the step never launched has no node)
    return true;
}

// replay: refresh the five nodes, launch
static int graph_step(mpmc_hip_ctx *c) {
    const DevAtoms a = dev_atoms(c);
    const DevBox bx = dev_box(c);
    timespec g0, g1, g2;
    clock_gettime(CLOCK_MONOTONIC, &g0);
    c->graph_mode = GM_UPDATE;
    // what the publish launch takes from the call: as the captured call left it (split stays false: a captured step joins
    // its two streams and publishes one record)
    c->call.do_polar = true;
    c->call.recip_chunks = c->sg.recip_chunks;
    c->call.res_zero_mask = c->sg.res_zero_mask;
    c->call.pair_rows_to_sum = c->sg.pair_rows_to_sum;
    int rc = flush_moves(c);
    if (!rc) rc = setup_view(c, c->view[0], a, bx, true, true, false);
    if (!rc) rc = launch_field(c, a, bx);
    if (!rc) rc = launch_pair_kernel(c, a, bx, c->stream2);
    if (!rc && c->sg.func[GS_RECIP]) rc = launch_recip_partial(c, a, c->stream2);
    c->energy_part = c->sg.energy_part;
    c->energy_nt = c->sg.energy_nt;
    if (!rc) rc = launch_publish(c);
    c->graph_mode = GM_DIRECT;
    if (rc) return -1;
    clock_gettime(CLOCK_MONOTONIC, &g1);
    HIPCHK(hipGraphLaunch(c->sg.exec, c->stream));
    clock_gettime(CLOCK_MONOTONIC, &g2);
    c->graph_update_s += (g1.tv_sec - g0.tv_sec) + 1e-9 * (g1.tv_nsec - g0.tv_nsec);
    c->graph_launch_s += (g2.tv_sec - g1.tv_sec) + 1e-9 * (g2.tv_nsec - g1.tv_nsec);
    c->result_view = c->sg.result_view;
    c->result_mu = c->sg.result_mu;
    c->psweep = c->sg.psweep;
    c->results_scattered = false;
    c->have_polar_result = true;
    c->call.iterations = c->sg.iterations;
    ++c->graph_launches;
    return 0;
}

extern "C" int mpmc_hip_energy(mpmc_hip_ctx *c, mpmc_hip_result *out) {
    if (mpmc_hip_energy_begin(c)) return -1;
    return mpmc_hip_energy_end(c, out);
}

// The combinations of modes an evaluation refuses, in the order they are checked (tests match on these strings).  Also where
// polarvdw's e_iso cache goes once the mode is off.
static int refuse_unsupported(mpmc_hip_ctx *c) {
    if (c->disp_on && c->rdc_order)
        return fail("MPMC_HIP: energy: rd_crystal with disp_expansion is not implemented (the reference's disp_expansion() "
                    "ignores rd_crystal)");
    if (c->rd_form) {
        if (c->disp_on)
            return fail("MPMC_HIP: energy: a pair potential of set_rd_form with disp_expansion (mpmc_hip_set_dispersion) is not "
                        "implemented");
        if (c->rdc_order)
            return fail("MPMC_HIP: energy: a pair potential of set_rd_form with rd_crystal (mpmc_hip_set_rd_crystal) is not "
                        "implemented");
        if (c->vdw_on)
            return fail("MPMC_HIP: energy: a pair potential of set_rd_form with polarvdw (mpmc_hip_set_vdw) is not implemented");
        if (c->rd_form != kRdFormSG && c->rd_mix == kRdMixWaldmanHagler && c->negative_sigma)
            return fail("MPMC_HIP: energy: waldmanhagler mixing with a negative sigma is refused (the reference never assigns "
                        "the epsilon of such a pair)");
        if (c->rd_form == kRdFormSG && c->rd_mix != kRdMixLB)
            return fail("MPMC_HIP: energy: the sg form takes no mixing rule (the reference ignores it there): set mixing lb");
    }
    if (c->have_params && c->par.polarization && !c->par.rd_only && c->thole_damp_type != 0 && !(c->par.polar_damp > 0.0))
        return fail("MPMC_HIP: energy: damping factor must be specified (polar_damp > 0) unless polar_damp_type is off");
    if (c->vdw_on) {
        if (c->thole_damp_type != 2 || c->thole_wolf_full)
            return fail("MPMC_HIP: energy: polarvdw with polar_damp_type linear / off or polar_wolf_full "
                        "(mpmc_hip_set_thole_model) is not implemented (the reference's e2body() / calc_e_iso() are written "
                        "for the exponential form)");
        if (c->disp_on)
            return fail("MPMC_HIP: energy: polarvdw with disp_expansion (mpmc_hip_set_dispersion) is not implemented");
        if (c->rdc_order)
            return fail("MPMC_HIP: energy: polarvdw with rd_crystal (mpmc_hip_set_rd_crystal) is not implemented");
        if (c->at_on)
            return fail("MPMC_HIP: energy: polarvdw with axilrod_teller (mpmc_hip_set_axilrod_teller) is not implemented");
        if (c->par.feynman_hibbs)
            return fail("MPMC_HIP: energy: polarvdw with feynman_hibbs is not implemented (the reference's finite-difference "
                        "correction cannot be matched)");
    } else {
        c->vdw_iso.clear();  // the mode is off: its e_iso cache goes
    }
    if (c->exact_polar && c->par.polarization && !c->par.rd_only) {
        if (c->par.polar_zodid)
            return fail("MPMC_HIP: energy: polar_zodid and polar_iterative are incompatible: the exact dipoles "
                        "(mpmc_hip_set_exact_polar) with polar_zodid are refused");  // check_input.c:349-353
        if (c->par.polar_palmo)
            return fail("MPMC_HIP: energy: the exact dipoles (mpmc_hip_set_exact_polar) with polar_palmo are not implemented "
                        "(the reference would add a stale ef_induced_change)");
        if (c->vdw_on)
            return fail("MPMC_HIP: energy: the exact dipoles (mpmc_hip_set_exact_polar) with polarvdw (mpmc_hip_set_vdw) are not "
                        "implemented (the reference forces the iterative solver there)");
    } else if (c->par.polarization && !c->par.rd_only && !c->par.polar_zodid && c->par.polar_precision == 0.0 &&
               c->par.polar_max_iter <= 0) {
        return fail("MPMC_HIP: polar_max_iter must be > 0 when polar_precision is 0");  // (accepted by set_params in the exact mode)
    }
    return 0;
}

// Enqueue the whole evaluation; nothing waits for the device (except the per-iteration convergence test
// of polar_precision mode), so the caller can do host work before mpmc_hip_energy_end() collects it.
extern "C" int mpmc_hip_energy_begin(mpmc_hip_ctx *c) {
    if (!c) return fail("MPMC_HIP: energy: null argument");
    if (c->in_flight) return fail("MPMC_HIP: energy_begin: the previous evaluation has not been collected");
    c->result_valid = false;
    if (!c->have_atoms) return fail("MPMC_HIP: energy: no configuration uploaded");
    if (!c->have_box) return fail("MPMC_HIP: energy: no box set");
    if (c->order_stale && gs_order_mode(c))
        return fail("MPMC_HIP: energy: Gauss-Seidel after insert_molecule / remove_molecule needs the sweep order of the "
                    "new configuration (mpmc_hip_set_sweep_order)");
    if (const int rc = refuse_unsupported(c)) return rc;
    if (!c->exact_polar) c->chol_nv = 0;
    HIPCHK(hipSetDevice(c->device));
    if (c->vdw_on && !c->par.rd_only && vdw_ensure_iso(c)) return -1;
    if (c->resident_off && c->resident_backoff > 0 && (long)c->energy_calls >= c->resident_retry_at)
        c->resident_off = false;  // (one more attempt at the one-launch solve; a give-up doubles the interval)
    const mpmc_hip_params &P = c->par;
    c->ewald_alpha = P.ewald_alpha_set ? P.ewald_alpha : 3.5 / c->cutoff;                    // pbc.c:73-74
    c->polar_ewald_alpha = P.polar_ewald_alpha_set ? P.polar_ewald_alpha : 3.5 / c->cutoff;  // pbc.c:75-76
    if (!P.rd_only && !P.wolf && (!c->kvec_valid || c->kvec_kmax != P.ewald_kmax)) {
        if (build_kvectors(c)) return -1;
        c->kvec_kmax = P.ewald_kmax;
    }
    timespec ts0, ts1;
    clock_gettime(CLOCK_MONOTONIC, &ts0);
    begin_call(c);
    bool issued = false;
    if (graph_eligible(c)) {
        if (c->sg.valid && c->sg.rev == c->config_rev) {
            if (graph_step(c)) return -1;
            issued = true;
        } else if (++c->eligible_streak >= 3) {
            // third steady-state step in a row: record this one
            graph_destroy(c);  // (also clears the slot table: a slot this step does not launch stays null)
            const MoveList saved = c->pending;
            bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                c->graph_mode = GM_CAPTURE;
                const int rc = enqueue_direct(c);
                c->graph_mode = GM_DIRECT;
                hipGraph_t graph = nullptr;
                ok = (hipStreamEndCapture(c->stream, &graph) == hipSuccess) && rc == 0 && graph != nullptr;
                if (ok) ok = graph_finish_capture(c, graph);
                else if (graph) hipGraphDestroy(graph);
            }
            if (ok) {
                c->sg.valid = true;
                c->sg.rev = c->config_rev;
                c->sg.iterations = c->call.iterations;
                c->sg.result_view = c->result_view;
                c->sg.result_mu = c->result_mu;
                c->sg.psweep = c->psweep;
                c->sg.energy_part = c->energy_part;
                c->sg.energy_nt = c->energy_nt;
                c->sg.recip_chunks = c->call.recip_chunks;
                c->sg.res_zero_mask = c->call.res_zero_mask;
                c->sg.pair_rows_to_sum = c->call.pair_rows_to_sum;
                HIPCHK(hipGraphLaunch(c->sg.exec, c->stream));
                ++c->graph_launches;
                issued = true;
            } else {
                // could not record: keep working launch by launch
                (void)hipGetLastError();
                graph_destroy(c);
                c->opt.graph = 0;
                c->pending = saved;
                c->call = CallState();  // (whatever the abandoned capture left)
                collect_dirty_blocks(c);
            }
        }
    } else {
        c->eligible_streak = 0;
    }
    if (!issued && enqueue_direct(c)) return -1;
    c->staged_copies = false;
    c->main_writes = false;
    clock_gettime(CLOCK_MONOTONIC, &ts1);
    c->host_enqueue_s += (ts1.tv_sec - ts0.tv_sec) + 1e-9 * (ts1.tv_nsec - ts0.tv_nsec);
    c->dirty_atoms.clear();
    c->all_dirty = false;
    c->in_flight = true;
    return 0;
}

// spin on a sequence number a publish kernel writes last; fall back to a stream sync if it does not show up (also
// surfaces launch errors)
static int wait_sequence(volatile double *seq, double want, hipStream_t stream) {
    for (unsigned long long spins = 0; spins < 2000000000ull; ++spins) {
        if (*seq == want) return 0;
        if ((spins & 0xfffffull) == 0xfffffull && hipStreamQuery(stream) != hipErrorNotReady) break;
        __builtin_ia32_pause();
    }
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
}

static int wait_record(mpmc_hip_ctx *c) {
    const double want = (double)c->energy_calls;
    if (wait_sequence(c->h_res + R_COUNT, want, c->stream)) return -1;
    // the side stream's part has a sequence number of its own
    return c->call.split ? wait_sequence(c->h_res2 + R_COUNT, want, c->stream2) : 0;
}

// energy_end(): the call it collected cannot be used; the same evaluation once more, with `flag` (what makes it take the
// other path) held true while it is enqueued
static int repeat_call(mpmc_hip_ctx *c, bool &flag) {
    flag = true;
    begin_call(c);
    const int rc = enqueue_direct(c);
    flag = false;
    return rc ? -1 : wait_record(c);
}

// The result of the call from the record(s) the publish kernels wrote (energy.c:149-196).
static void assemble_result(mpmc_hip_ctx *c, int iter_success, mpmc_hip_result *out) {
    const mpmc_hip_params &P = c->par;
    const bool do_polar = c->call.do_polar;
    const int polar_iterations = c->call.iterations;
    double r[R_COUNT];
    for (int k = 0; k < R_COUNT; ++k) r[k] = (c->call.split && ((kSideSlots >> k) & 1u)) ? c->h_res2[k] : c->h_res[k];
    // (disp_expansion: the LJ kernels ran on zero parameters, both of their slots are exactly 0)
    // (rd_crystal: the same, with the image sum, its self part and the correction at cutoff_c behind them)
    const double rd = c->disp_on     ? (r[R_RD_PAIR] + r[R_LRC]) + (r[R_DISP] + r[R_DISP_LRC])
                      : c->rdc_order ? (r[R_RD_PAIR] + r[R_LRC]) + ((r[R_DISP] + r[R_RDC_SELF]) + r[R_DISP_LRC])
                      : c->vdw_on    ? (r[R_RD_PAIR] + r[R_LRC]) + (r[R_DISP] + r[R_DISP_LRC])  // polarvdw: repulsion only
                      : c->rd_form   ? (r[R_RD_PAIR] + r[R_LRC]) + (r[R_DISP] + r[R_DISP_LRC])  // set_rd_form: the same slots
                                     : r[R_RD_PAIR] + r[R_LRC];
    const double real = r[R_ES_REAL] - r[R_ES_INTRA];
    const bool ewald = !P.rd_only && !P.wolf;
    const double recip = ewald ? r[R_RECIP] * (4.0 * kPI / c->volume) : 0.0;  // coulombic.c:92
    const double self = ewald ? r[R_SELF] : 0.0;
    const double coul = P.rd_only ? 0.0 : real + recip + self;  // coulombic.c:36
    const double upol = do_polar ? r[R_UPOL] : 0.0;
    out->rd_energy = rd;
    out->es_real = P.rd_only ? 0.0 : real;
    out->es_recip = recip;
    out->es_self = self;
    out->coulombic_energy = coul;
    out->polarization_energy = upol;
    out->energy = rd + coul + upol;  // energy.c:196
    c->three_body = c->at_on ? r[R_AT] : 0.0;
    if (c->at_on) out->energy += c->three_body;  // energy.c:194: behind the other terms (vdw_energy is 0 on this path)
    // polarvdw: vdw_energy = e_total - e_iso + lr_corr (vdw.c:631; not under rd_only), added at energy.c:194-196
    c->vdw_energy = (c->vdw_on && !P.rd_only) ? ((r[R_VDW] - c->vdw_e_iso) + 0.0) + r[R_VDW_LRC] : 0.0;
    if (c->vdw_on) out->energy += c->vdw_energy;
    c->vdw_terms[0] = (c->vdw_on && !P.rd_only) ? r[R_VDW] : 0.0;
    c->vdw_terms[1] = (c->vdw_on && !P.rd_only) ? c->vdw_e_iso : 0.0;
    c->vdw_terms[2] = (c->vdw_on && !P.rd_only) ? r[R_VDW_LRC] : 0.0;
    c->vdw_terms[3] = c->vdw_on ? r[R_DISP] : 0.0;
    c->vdw_terms[4] = c->vdw_on ? r[R_DISP_LRC] : 0.0;
    c->close_contacts = c->autoreject_scale != 0.0 ? (long long)r[R_CONTACTS] : 0;
    out->dipole_rrms = (do_polar && !c->call.exact) ? r[R_RRMS] : 0.0;
    out->volume = c->volume;
    out->cutoff = c->cutoff;
    out->ewald_alpha = c->ewald_alpha;
    out->polar_ewald_alpha = c->polar_ewald_alpha;
    out->polar_iterations = polar_iterations;
    out->iter_success = iter_success;
    out->n_atoms = c->n_valid;
    out->status = std::isfinite(out->energy) ? 0 : 1;
}

extern "C" int mpmc_hip_energy_end(mpmc_hip_ctx *c, mpmc_hip_result *out) {
    if (!c || !out) return fail("MPMC_HIP: energy: null argument");
    if (!c->in_flight) return fail("MPMC_HIP: energy_end: no evaluation in flight");
    c->in_flight = false;
    memset(out, 0, sizeof(*out));
    timespec ts1, ts2;
    clock_gettime(CLOCK_MONOTONIC, &ts1);
    if (wait_record(c)) return -1;
    if (c->call.spec_rank && c->h_res[R_GS_ERR] == 0.0 && c->h_res[R_RANKCHG] != 0.0) {
        // polar_gs_ranked, speculative call: the ranking metric is not the one the resident ranked view was built
        // for (molecules came within 1.5 r_min of each other, or moved apart again).  Nothing that call produced is
        // used; the evaluation is repeated with the host sorting the new metric (which rebuilds the ranked view).
        // Everything else resident -- pair / field partials, view 0 -- is already up to date and is not redone.
        ++c->spec_redos;
        if (repeat_call(c, c->force_host_rank)) return -1;
    }
    if (c->call.resident && c->h_res[R_GS_ERR] != 0.0) {
        // The resident Jacobi launch gave up on a hand-off (its workgroups were not all running at once: the device
        // is shared with another process, or a test asked for it).  Nothing it produced is used: the evaluation is
        // repeated on the multi-launch path, which this context then keeps to; the partial-sum slots are refilled
        // before the resident kernel could ever run again.
        ++c->resident_fallbacks;
        c->resident_off = true;
        // a shared device may be free again later: one more attempt after `backoff` clean calls (a failed attempt costs
        // the bounded waits, ~0.2 s, so the interval doubles every time it fails)
        c->resident_backoff = c->resident_backoff ? std::min(2 * c->resident_backoff, 1L << 20) : 4096;
        c->resident_retry_at = (long)c->energy_calls + c->resident_backoff;
        c->view[0].resP_armed = false;
        if (repeat_call(c, c->force_multi_launch)) return -1;
    }
    clock_gettime(CLOCK_MONOTONIC, &ts2);
    c->host_wait_s += (ts2.tv_sec - ts1.tv_sec) + 1e-9 * (ts2.tv_nsec - ts1.tv_nsec);
    const bool timed_call = c->call.timed;
    // (exact dipoles: the factorization's flag word came with the record, in the slot the iterative paths keep <rrms> in)
    const int iter_success = c->call.exact ? (c->h_res[R_RRMS] != 0.0 ? 1 : 0) : c->call.iter_success;
    if (c->call.exact) {
        c->chol_done = true;
        c->chol_failed = iter_success != 0;
    }
    const int gs_err = (int)c->h_res[R_GS_ERR];
    c->h_gserr[0] = gs_err & 1;
    c->h_gserr[1] = (gs_err >> 1) & 1;
    const bool gs_timeout = gs_err != 0;
    if (gs_timeout) {
        unsigned dbg[8] = {0};
        const SweepView &gv = c->view[c->h_gserr[1] ? 1 : 0];
        hipMemcpy(dbg, gv.gsflags, sizeof(dbg), hipMemcpyDeviceToHost);  // (the allocation is exactly 8 words)
        return fail("MPMC_HIP: persistent Gauss-Seidel kernel gave up waiting on a hand-off (spin limit) in view %d: "
                    "workgroup %u thread %u addr-lo 0x%x; mu_new-lo 0x%x",
                    c->h_gserr[1] ? 1 : 0, dbg[2], dbg[3], dbg[4], (unsigned)((unsigned long long)gv.mupub.get() & 0xffffffffu));
    }
    HIPCHK(hipGetLastError());
    c->timed = timed_call;
    c->stage_used = 0;
    assemble_result(c, iter_success, out);
    c->last_result = *out;
    c->result_rev = c->config_rev;
    c->result_valid = true;
    return 0;
}

extern "C" int mpmc_hip_download_dipoles(mpmc_hip_ctx *c, double *mu, double *ef_static, double *ef_induced,
                                         double *ef_induced_change) {
    if (!c || !c->have_atoms) return fail("MPMC_HIP: download_dipoles: no configuration");
    if (!c->have_polar_result) return fail("MPMC_HIP: download_dipoles: no polarization energy evaluated yet");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_static_field(c)) return -1;
    if (complete_pending_sweep(c)) return -1;  // mu_n and E_ind(mu_{n-1}), if the call left its last sweeps to this moment
    if (!c->results_scattered) {
        // the solver works on the compacted polarizable atoms; atom order is produced when somebody asks
        SweepView *V = c->result_view;
        hipLaunchKernelGGL(scatter_results_kernel, dim3((c->npad + 255) / 256), dim3(256), 0, c->stream, c->npad,
                           V->d_slot, c->result_mu, V->efind, V->efchg, c->d_mu, c->d_efind, c->d_efchg);
        HIPCHK(hipStreamSynchronize(c->stream));
        c->results_scattered = true;
    }
    const size_t b = 3 * (size_t)c->n * sizeof(double);
    if (mu) HIPCHK(hipMemcpy(mu, c->d_mu, b, hipMemcpyDeviceToHost));
    if (ef_static) HIPCHK(hipMemcpy(ef_static, c->d_es, b, hipMemcpyDeviceToHost));
    if (ef_induced) HIPCHK(hipMemcpy(ef_induced, c->d_efind, b, hipMemcpyDeviceToHost));
    if (ef_induced_change) HIPCHK(hipMemcpy(ef_induced_change, c->d_efchg, b, hipMemcpyDeviceToHost));
    return 0;
}

// The solver keeps only the polarizable block of A on the device; the full 3N x 3N matrix of the
// reference (system->A_matrix, read e.g. by vdw.c:244) is produced here on demand.
extern "C" int mpmc_hip_download_amatrix(mpmc_hip_ctx *c, double *A) {
    if (!c || !c->have_atoms || !c->have_box || !A) return fail("MPMC_HIP: download_amatrix: no configuration");
    HIPCHK(hipSetDevice(c->device));
    const size_t n3 = 3 * (size_t)c->n, lda = 3 * (size_t)c->npad;
    if (flush_moves(c)) return -1;
    DevBuf<double> dA;
    HIPCHK(dA.alloc(lda * lda));
    MPMC_THOLE_DISPATCH(c, hipLaunchKernelGGL((build_amatrix_kernel<kM>), dim3(c->npad / 128, c->npad / kARows), dim3(64), 0,
                                              c->stream, dev_atoms(c), dev_box(c), thole_params(c, nullptr), dA, (int)lda));
    hipError_t e = hipMemcpy2DAsync(A, n3 * sizeof(double), dA, lda * sizeof(double), n3 * sizeof(double), n3,
                                    hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail("MPMC_HIP: download_amatrix: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int mpmc_hip_download_ranking(mpmc_hip_ctx *c, double *rank_metric, int *ranked_array) {
    if (!c || !c->have_atoms) return fail("MPMC_HIP: download_ranking: no configuration");
    HIPCHK(hipSetDevice(c->device));
    if (rank_metric) HIPCHK(hipMemcpy(rank_metric, c->d_rank, c->n * sizeof(double), hipMemcpyDeviceToHost));
    if (ranked_array) {
        // the reference's ranked_array after update_ranking() (thole_iterative.c:143-164): a stable descending sort of
        // the identity by the metric -- made here, on demand, from the metric the last ranked call was sorted from
        std::vector<int> perm(c->n);
        std::iota(perm.begin(), perm.end(), 0);
        // ... of the order the sweeps started from: after insert / remove that is the order the caller stated
        // (mpmc_hip_set_sweep_order), not the slot order.  The polarizable sites take, in the stated order, the places the
        // polarizable sites have in slot order (the identity while the view is the upload's).
        const SweepView &v0 = c->view[0];
        if (gs_order_mode(c) && !c->order_stale && (int)v0.slot_of_atom.size() == c->n) {
            size_t k = 0;
            for (int a = 0; a < c->n && k < v0.h_idx.size(); ++a)
                if (v0.slot_of_atom[a] >= 0) perm[a] = v0.h_idx[k++];
        }
        if (c->perm_ranked && (int)c->rank_saved.size() == c->n) {
            const double *rk = c->rank_saved.data();
            std::stable_sort(perm.begin(), perm.end(), [rk](int x, int y) { return rk[x] > rk[y]; });
        }
        memcpy(ranked_array, perm.data(), c->n * sizeof(int));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// CavityGrid: the grid of cavity_bias (kernels_cavity.h).  State of the context that nothing but
// these calls and a box change touches: it knows no atom slot, so upload(), update_atoms(), insert / remove and energy()
// leave it alone.  Everything runs on the main stream; update and point wait for their record.
// ---------------------------------------------------------------------------------------------
// the smallest double T with sqrt(T) >= radius: sqrt(s) < radius <=> s < T for every s (sqrt is monotone)
static double cavity_threshold(double radius) {
    double t = radius * radius;
    while (std::sqrt(t) < radius) t = std::nextafter(t, INFINITY);
    for (;;) {
        const double below = std::nextafter(t, 0.0);
        if (below == t || std::sqrt(below) < radius) break;
        t = below;
    }
    return t;
}

static int cavity_grid_dim(const mpmc_hip_ctx *c) { return (c->cav_P + kCavThreads - 1) / kCavThreads; }

static int cavity_ensure_points(mpmc_hip_ctx *c) {
    if (c->cav_pos_valid) return 0;
    if (!c->have_box) return fail("MPMC_HIP: cavity grid: no box set");
    CavityFrac f;
    memset(&f, 0, sizeof(f));
    for (int i = 0; i < c->cav_G; ++i) f.c[i] = ((double)(i + 1)) / ((double)(c->cav_G + 1));
    CavityBasis bs;
    memcpy(bs.b, c->basis, sizeof(bs.b));
    hipLaunchKernelGGL(cavity_points_kernel, dim3(cavity_grid_dim(c)), dim3(kCavThreads), 0, c->stream, c->cav_G, f, bs,
                       c->d_cav_pos.get(), c->d_cav_pos.get() + c->cav_P, c->d_cav_pos.get() + 2 * (size_t)c->cav_P);
    HIPCHK(hipGetLastError());
    c->cav_pos_valid = true;
    return 0;
}

// `count` doubles from the caller to `dst` through the pinned staging buffer; the caller of this waits for the stream
// before the staging buffer is filled again
static int cavity_stage(mpmc_hip_ctx *c, DevBuf<double> &dst, const double *const *src, const size_t *len, int nsrc) {
    size_t count = 0;
    for (int k = 0; k < nsrc; ++k) count += len[k];
    if (count == 0) return 0;
    if (dst.size() < count || c->h_cav_stage.size() < count) {
        HIPCHK(hipStreamSynchronize(c->stream));  // (growth only: an earlier launch may still read the old buffer)
        if (dst.size() < count) HIPCHK(dst.alloc(count + count / 2));
        if (c->h_cav_stage.size() < count) HIPCHK(c->h_cav_stage.alloc(count + count / 2));
    }
    size_t at = 0;
    for (int k = 0; k < nsrc; ++k) {
        memcpy(c->h_cav_stage + at, src[k], len[k] * sizeof(double));
        at += len[k];
    }
    HIPCHK(hipMemcpyAsync(dst, c->h_cav_stage, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return 0;
}

extern "C" int mpmc_hip_set_cavity_grid(mpmc_hip_ctx *c, int grid_size, double radius) {
    if (!c) return fail("MPMC_HIP: set_cavity_grid: null context");
    if (c->in_flight) return fail("MPMC_HIP: set_cavity_grid between energy_begin() and energy_end()");
    if (grid_size < 0 || grid_size > kCavMaxGrid)
        return fail("MPMC_HIP: set_cavity_grid: cavity_grid %d is not supported (1 .. %d; 0 = off)", grid_size, kCavMaxGrid);
    if (grid_size > 0 && (!(radius > 0.0) || !std::isfinite(radius)))
        return fail("MPMC_HIP: set_cavity_grid: invalid cavity grid or radius specified (cavity_radius %g)", radius);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));  // (an earlier launch may still read the buffers replaced below)
    c->cav_pos_valid = c->cav_occ_valid = false;
    c->cav_open = -1;
    if (grid_size == 0) {
        c->cav_G = c->cav_P = 0;
        c->d_cav_pos.reset();
        c->d_cav_occ.reset();
        c->d_cav_open.reset();
        c->d_cav_blk.reset();
        return 0;
    }
    const size_t P = (size_t)grid_size * grid_size * grid_size;
    c->cav_G = 0;  // (off, should an allocation below fail)
    if (c->d_cav_pos.size() != 3 * P) {
        HIPCHK(c->d_cav_pos.alloc(3 * P));
        HIPCHK(c->d_cav_occ.alloc(P));
        HIPCHK(c->d_cav_open.alloc(P));
        HIPCHK(c->d_cav_blk.alloc(2 * ((P + kCavThreads - 1) / kCavThreads)));
    }
    if (!c->d_cav_cnt) HIPCHK(c->d_cav_cnt.alloc(CAV_NCOUNTER));
    if (!c->h_cav) {
        HIPCHK(c->h_cav.alloc(CR_COUNT, hipHostMallocMapped));
        memset(c->h_cav, 0, CR_COUNT * sizeof(double));
        HIPCHK(hipHostGetDevicePointer((void **)&c->h_cav_dev, c->h_cav, 0));
    }
    c->cav_G = grid_size;
    c->cav_P = (int)P;
    c->cav_radius = radius;
    c->cav_T = cavity_threshold(radius);
    return 0;
}

static int cavity_check(mpmc_hip_ctx *c, const char *what) {
    if (!c) return fail("MPMC_HIP: %s: null context", what);
    if (c->in_flight) return fail("MPMC_HIP: %s between energy_begin() and energy_end()", what);
    if (c->cav_G == 0) return fail("MPMC_HIP: %s: the cavity grid is off (mpmc_hip_set_cavity_grid)", what);
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

extern "C" int mpmc_hip_cavity_bin(mpmc_hip_ctx *c, int n, const double *x, const double *y, const double *z) {
    if (cavity_check(c, "cavity_bin")) return -1;
    if (n < 0) return fail("MPMC_HIP: cavity_bin: n = %d", n);
    if (n > 0 && (!x || !y || !z)) return fail("MPMC_HIP: cavity_bin: null argument");
    if (cavity_ensure_points(c)) return -1;
    c->cav_occ_valid = false;
    c->cav_open = -1;
    const double *src[3] = {x, y, z};
    const size_t len[3] = {(size_t)n, (size_t)n, (size_t)n};
    if (cavity_stage(c, c->d_cav_atoms, src, len, 3)) return -1;
    const double *a = c->d_cav_atoms, *g = c->d_cav_pos;
    const size_t P = (size_t)c->cav_P;
    hipLaunchKernelGGL(cavity_bin_kernel, dim3(cavity_grid_dim(c)), dim3(kCavThreads), 0, c->stream, c->cav_P, g, g + P,
                       g + 2 * P, n, a, a + n, a + 2 * (size_t)n, c->cav_T, c->d_cav_occ.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));  // (the staging buffer is free again; a full bin is the rare path)
    c->cav_occ_valid = true;
    return 0;
}

extern "C" int mpmc_hip_cavity_update(mpmc_hip_ctx *c, int n_out, const double *out_xyz, int n_in, const double *in_xyz,
                                      int n_darts, const double *dart_xyz, int *cavities_open, int *hits) {
    if (cavity_check(c, "cavity_update")) return -1;
    if (n_out < 0 || n_in < 0 || n_darts < 0)
        return fail("MPMC_HIP: cavity_update: negative count (%d out, %d in, %d darts)", n_out, n_in, n_darts);
    if ((n_out > 0 && !out_xyz) || (n_in > 0 && !in_xyz) || (n_darts > 0 && !dart_xyz) || !cavities_open || !hits)
        return fail("MPMC_HIP: cavity_update: null argument");
    if (!c->cav_occ_valid || n_out > kCavMaxEdit || n_in > kCavMaxEdit) return 1;
    if (n_out + n_in > 0 && !c->cav_incremental) return 1;
    CavityEdit ed;
    memset(&ed, 0, sizeof(ed));
    ed.n_out = n_out;
    ed.n_in = n_in;
    if (n_out > 0) memcpy(ed.out, out_xyz, 3 * (size_t)n_out * sizeof(double));
    if (n_in > 0) memcpy(ed.in, in_xyz, 3 * (size_t)n_in * sizeof(double));
    const size_t nd = 3 * (size_t)n_darts;
    if (cavity_stage(c, c->d_cav_darts, &dart_xyz, &nd, 1)) return -1;
    if (c->d_cav_dart_hit.size() < (size_t)n_darts) {
        HIPCHK(hipStreamSynchronize(c->stream));  // (growth only)
        HIPCHK(c->d_cav_dart_hit.alloc((size_t)n_darts + (size_t)n_darts / 2));
    }
    const double *g = c->d_cav_pos;
    const size_t P = (size_t)c->cav_P;
    const int nb = cavity_grid_dim(c);
    int *blk_open = c->d_cav_blk, *blk_off = c->d_cav_blk.get() + nb;
    hipLaunchKernelGGL(cavity_edit_kernel, dim3(nb), dim3(kCavThreads), 0, c->stream, c->cav_P, g, g + P, g + 2 * P, ed,
                       c->cav_T, c->d_cav_occ.get(), blk_open);
    hipLaunchKernelGGL(cavity_scan_kernel, dim3(1), dim3(kCavThreads), 0, c->stream, nb, (const int *)blk_open, blk_off,
                       c->d_cav_cnt.get(), n_darts, c->d_cav_dart_hit.get());
    hipLaunchKernelGGL(cavity_scatter_kernel, dim3(nb), dim3(kCavThreads), 0, c->stream, c->cav_P,
                       (const int *)c->d_cav_occ, (const int *)blk_off, c->d_cav_open.get());
    if (n_darts > 0) {
        // the open list is shared out over enough workgroups to fill the device: the darts alone are too few waves
        const int dart_blocks = (n_darts + kCavThreads - 1) / kCavThreads;
        const int slices = std::max(1, std::min(nb, (4 * c->num_cus + dart_blocks - 1) / dart_blocks));
        hipLaunchKernelGGL(cavity_darts_kernel, dim3(dart_blocks, slices), dim3(kCavThreads), 0, c->stream, n_darts,
                           (const double *)c->d_cav_darts, (const int *)c->d_cav_open, g, g + P, g + 2 * P, c->cav_T,
                           (const int *)c->d_cav_cnt, c->d_cav_dart_hit.get());
    }
    const double seq = (double)++c->cav_seq;
    hipLaunchKernelGGL(cavity_publish_kernel, dim3(1), dim3(kCavThreads), 0, c->stream, n_darts,
                       (const int *)c->d_cav_dart_hit, (const int *)c->d_cav_cnt, c->h_cav_dev, seq);
    HIPCHK(hipGetLastError());
    if (wait_sequence(c->h_cav + CR_SEQ, seq, c->stream)) return -1;
    if (c->h_cav[CR_SEQ] != seq) return fail("MPMC_HIP: cavity_update: the record did not arrive");
    c->cav_open = (int)c->h_cav[CR_OPEN];
    *cavities_open = c->cav_open;
    *hits = (int)c->h_cav[CR_HITS];
    return 0;
}

extern "C" int mpmc_hip_cavity_point(mpmc_hip_ctx *c, int index, int *grid_index, double pos[3]) {
    if (cavity_check(c, "cavity_point")) return -1;
    if (!grid_index || !pos) return fail("MPMC_HIP: cavity_point: null argument");
    if (c->cav_open < 0) return fail("MPMC_HIP: cavity_point: no cavity_update since the occupancy was replaced");
    if (index < 0 || index >= c->cav_open)
        return fail("MPMC_HIP: cavity_point: index %d outside the %d open points", index, c->cav_open);
    const double *g = c->d_cav_pos;
    const size_t P = (size_t)c->cav_P;
    const double seq = (double)++c->cav_seq;
    hipLaunchKernelGGL(cavity_pick_kernel, dim3(1), dim3(64), 0, c->stream, index, (const int *)c->d_cav_open, g, g + P,
                       g + 2 * P, c->h_cav_dev, seq);
    HIPCHK(hipGetLastError());
    if (wait_sequence(c->h_cav + CR_SEQ, seq, c->stream)) return -1;
    if (c->h_cav[CR_SEQ] != seq) return fail("MPMC_HIP: cavity_point: the record did not arrive");
    *grid_index = (int)c->h_cav[CR_PICK_G];
    for (int p = 0; p < 3; ++p) pos[p] = c->h_cav[CR_PICK_X + p];
    return 0;
}

extern "C" int mpmc_hip_download_cavity_grid(mpmc_hip_ctx *c, int *occupancy, double *pos) {
    if (cavity_check(c, "download_cavity_grid")) return -1;
    if (!occupancy && !pos) return fail("MPMC_HIP: download_cavity_grid: null argument");
    const size_t P = (size_t)c->cav_P;
    if (occupancy) {
        if (!c->cav_occ_valid) return fail("MPMC_HIP: download_cavity_grid: no occupancy (mpmc_hip_cavity_bin) for this grid and box");
        HIPCHK(hipMemcpyAsync(occupancy, c->d_cav_occ, P * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    if (pos) {
        if (cavity_ensure_points(c)) return -1;
        std::vector<double> soa(3 * P);
        HIPCHK(hipMemcpyAsync(soa.data(), c->d_cav_pos, 3 * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (size_t g = 0; g < P; ++g)
            for (int p = 0; p < 3; ++p) pos[3 * g + p] = soa[p * P + g];
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static_assert(kDimerChunk == MPMC_HIP_DIMER_CHUNK && kDimerNotConverged == MPMC_HIP_DIMER_NOT_CONVERGED,
              "kernels_dimer.h and mpmc_hip.h disagree");
#include "engine_dimer.inc"
#include "engine_trial.inc"

extern "C" int mpmc_hip_get_timings(mpmc_hip_ctx *c, mpmc_hip_timings *t) {
    if (!c || !t) return fail("MPMC_HIP: get_timings: null argument");
    memset(t, 0, sizeof(*t));
    t->graph_steps = (int)c->graph_launches;
    t->spec_rank_redos = (int)c->spec_redos;
    t->resident_calls = (int)c->resident_calls;
    t->resident_fallbacks = (int)c->resident_fallbacks;
    t->pending_sweeps = (int)c->psweep.sweeps.size();  // (state, not an event measurement)
    if (!c->timed) return 0;
    HIPCHK(hipSetDevice(c->device));
    float acc[T_NCLASS] = {0};
    int cnt[T_NCLASS] = {0};
    for (const TimeRec &r : c->recs) {
        float ms = 0.f;
        HIPCHK(hipEventSynchronize(r.b));
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        acc[r.cls] += ms;
        cnt[r.cls]++;
    }
    t->pair_ms = acc[T_PAIR];
    t->recip_ms = acc[T_RECIP];
    t->field_ms = acc[T_FIELD];
    t->amatrix_ms = acc[T_AMAT];
    t->sweep_ms = acc[T_SWEEP];
    t->palmo_ms = acc[T_PALMO];
    t->other_ms = acc[T_OTHER];
    t->sweep_count = cnt[T_SWEEP];
    t->amatrix_count = cnt[T_AMAT];
    t->event_pair_ms = acc[T_EVPAIR];
    t->event_pair_count = cnt[T_EVPAIR];
    float tot = 0.f;
    HIPCHK(hipEventElapsedTime(&tot, c->ev_first, c->ev_last));
    t->total_ms = tot;
    return 0;
}

// ------------------------------------------------------------------------------------------
// RCCL (xGMI) averaging of walker observables.  librccl is bound lazily so that the energy
// path has no hard dependency on it.
// ------------------------------------------------------------------------------------------
struct Rccl {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                              hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static Rccl g_rccl;

struct mpmc_hip_comm {
    HipStream stream;              // of its own: the collective never queues behind (or in front of) an energy()
    ncclComm_t nccl = nullptr;
    int device = 0;                // (not the context: a caller may replace its context, e.g. when uvt outgrows it)
    DevBuf<double> d_buf;
    PinnedBuf<double> h_buf;       // pinned staging, so that both copies are truly asynchronous
    int nranks = 1, rank = 0;
    int pending = 0;               // doubles of the all-reduce in flight (0: none)
    DevBuf<unsigned char> d_gather;  // mpmc_hip_gather_observables: [send | nranks records]
    PinnedBuf<unsigned char> h_gather;
    // (the caller has set the device; the members free the buffers, then the stream)
    ~mpmc_hip_comm() {
        if (stream) hipStreamSynchronize(stream);
        if (nccl) g_rccl.CommDestroy(nccl);
    }
};

static int load_rccl() {
    if (g_rccl.h) return 0;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail("MPMC_HIP: cannot load librccl: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(h, "ncclAllGather");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail("MPMC_HIP: librccl lacks an expected symbol");
    g_rccl.h = h;
    return 0;
}

static int rccl_fail(const char *what, ncclResult_t rc) {
    return fail("MPMC_HIP: %s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "?");
}

extern "C" int mpmc_hip_comm_unique_id(unsigned char id[128]) {
    if (load_rccl()) return -1;
    ncclUniqueId u;
    static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is 128 bytes");
    const ncclResult_t rc = g_rccl.GetUniqueId(&u);
    if (rc != ncclSuccess) return rccl_fail("ncclGetUniqueId", rc);
    memcpy(id, u.internal, 128);
    return 0;
}

extern "C" int mpmc_hip_comm_create(mpmc_hip_comm **out, mpmc_hip_ctx *ctx, int nranks, int rank,
                                    const unsigned char id[128]) {
    if (!out || !ctx || !id || nranks <= 0 || rank < 0 || rank >= nranks)
        return fail("MPMC_HIP: comm_create: bad arguments");
    if (load_rccl()) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<mpmc_hip_comm> cm(new mpmc_hip_comm());  // (an early return below frees what was made)
    cm->device = ctx->device;
    cm->nranks = nranks;
    cm->rank = rank;
    ncclUniqueId u;
    memcpy(u.internal, id, 128);
    ncclComm_t nccl = nullptr;  // (cm destroys it only once the init has succeeded)
    const ncclResult_t rc = g_rccl.CommInitRank(&nccl, nranks, u, rank);
    if (rc != ncclSuccess) return rccl_fail("ncclCommInitRank", rc);
    cm->nccl = nccl;
    HIPCHK(hipStreamCreateWithFlags(cm->stream.out(), hipStreamNonBlocking));
    HIPCHK(cm->d_buf.alloc(64));
    HIPCHK(cm->h_buf.alloc(64));
    *out = cm.release();
    return 0;
}

extern "C" int mpmc_hip_comm_size(const mpmc_hip_comm *cm) { return cm ? cm->nranks : 0; }
extern "C" int mpmc_hip_comm_rank(const mpmc_hip_comm *cm) { return cm ? cm->rank : -1; }

// Sum over walkers of a small observable vector (<= 64 doubles), in two halves: _begin copies the values out
// of the caller's buffer and launches copy-in / all-reduce / copy-out on the communicator's own stream, _end
// waits for them and writes the sums.  The averages are only reported, never fed back into the chains, so a
// caller can run the next corrtime interval's energy() calls in between (the reference blocks in MPI_Gather,
// mc.c:431).  One collective in flight per communicator.
extern "C" int mpmc_hip_allreduce_observables_begin(mpmc_hip_comm *cm, const double *values, int count) {
    if (!cm || !values || count <= 0 || (size_t)count > cm->d_buf.size()) return fail("MPMC_HIP: allreduce: bad arguments");
    if (cm->pending) return fail("MPMC_HIP: allreduce_begin: the previous all-reduce has not been collected");
    HIPCHK(hipSetDevice(cm->device));
    memcpy(cm->h_buf, values, count * sizeof(double));
    HIPCHK(hipMemcpyAsync(cm->d_buf, cm->h_buf, count * sizeof(double), hipMemcpyHostToDevice, cm->stream));
    const ncclResult_t rc =
        g_rccl.AllReduce(cm->d_buf, cm->d_buf, (size_t)count, ncclFloat64, ncclSum, cm->nccl, cm->stream);
    if (rc != ncclSuccess) return rccl_fail("ncclAllReduce", rc);
    HIPCHK(hipMemcpyAsync(cm->h_buf, cm->d_buf, count * sizeof(double), hipMemcpyDeviceToHost, cm->stream));
    cm->pending = count;
    return 0;
}

extern "C" int mpmc_hip_allreduce_observables_end(mpmc_hip_comm *cm, double *values) {
    if (!cm || !values) return fail("MPMC_HIP: allreduce: bad arguments");
    if (!cm->pending) return fail("MPMC_HIP: allreduce_end: no all-reduce in flight");
    HIPCHK(hipSetDevice(cm->device));
    const int count = cm->pending;
    cm->pending = 0;
    HIPCHK(hipStreamSynchronize(cm->stream));
    memcpy(values, cm->h_buf, count * sizeof(double));
    return 0;
}

// the blocking form, in place
extern "C" int mpmc_hip_allreduce_observables(mpmc_hip_comm *cm, double *values, int count) {
    if (mpmc_hip_allreduce_observables_begin(cm, values, count)) return -1;
    return mpmc_hip_allreduce_observables_end(cm, values);
}

// The reference's MPI_Gather of one byte record per walker (mc.c:431), as an all-gather: every rank ends up with
// all records in rank order.  Blocking; staged through pinned memory on the communicator's own stream.
extern "C" int mpmc_hip_gather_observables(mpmc_hip_comm *cm, const void *record, int bytes, void *records) {
    if (!cm || !record || !records || bytes <= 0) return fail("MPMC_HIP: gather: bad arguments");
    if (cm->pending) return fail("MPMC_HIP: gather: an all-reduce is in flight on this communicator");
    HIPCHK(hipSetDevice(cm->device));
    const size_t b = (size_t)bytes, need = b * (size_t)(cm->nranks + 1);
    if (cm->d_gather.size() < need || cm->h_gather.size() < need) {
        HIPCHK(cm->d_gather.alloc(need));
        HIPCHK(cm->h_gather.alloc(need));
    }
    memcpy(cm->h_gather, record, b);
    HIPCHK(hipMemcpyAsync(cm->d_gather, cm->h_gather, b, hipMemcpyHostToDevice, cm->stream));
    const ncclResult_t rc = g_rccl.AllGather(cm->d_gather, cm->d_gather + b, b, ncclChar, cm->nccl, cm->stream);
    if (rc != ncclSuccess) return rccl_fail("ncclAllGather", rc);
    HIPCHK(hipMemcpyAsync(cm->h_gather + b, cm->d_gather + b, b * cm->nranks, hipMemcpyDeviceToHost, cm->stream));
    HIPCHK(hipStreamSynchronize(cm->stream));
    memcpy(records, cm->h_gather + b, b * cm->nranks);
    return 0;
}

extern "C" void mpmc_hip_comm_destroy(mpmc_hip_comm *cm) {
    if (!cm) return;
    hipSetDevice(cm->device);
    delete cm;
}
