// emi_args.hpp -- tile constants and kernel argument blocks.  Shared by the kernels built into
// libemi355x.so and by the model programs compiled at run time (emi_rtc.hip), so it stays free of
// host-only includes.
#pragma once
#ifdef __HIPCC_RTC__
// values of include/emi355x.h (checked against it on the static side, emi_kernels.hpp)
#define EMI_PATH_ELLIPSE 0
#define EMI_PATH_DISC 1
#define EMI_PATH_TRACK 2
#define EMI_PATH_REC 8
#else
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "emi355x.h"
#endif

#define EMI_NODE_THREADS 256

// Memory order of the arrival tickets (COST finish of the node role, split-K combine of the MFMA role).  The partial sums
// travel as agent-scope (sc1: write-through, L1- and L2-line-dropping) stores, every storing wave drains vmcnt, a workgroup
// barrier, then ONE lane's agent-scope atomic add on the ticket; the workgroup whose add came last reads them back with
// agent-scope (sc1) loads -- row 1 of the hand-off table of MI355X_MICROARCH.md ("Valid forms"), measured valid on gfx950.
// The ticket itself stays RELAXED: as ACQ_REL its release half is `buffer_wbl2 sc1`, a write-back of the XCD's whole L2,
// issued once per node workgroup under the pass's 1 GB store stream -- measured on one box, same process: 0.2848 ms per
// pass against 0.2243 at 1024 instances, 0.0433 against 0.0347 at 128 (tools/ab_build.sh relaxed; profiles/r03_notes.md).
// -DEMI_TICKET_ACQ_REL builds the fenced form (ordering by the HIP memory model rather than by the ISA's cache behaviour).
#ifdef EMI_TICKET_ACQ_REL
#define EMI_TICKET_ORDER __ATOMIC_ACQ_REL
#else
#define EMI_TICKET_ORDER __ATOMIC_RELAXED
#endif
// one wait state between an SALU write of m0 and an LDS-DMA instruction (-DEMI_NO_M0_NOP: the round-2 form, A/B only)
#ifdef EMI_NO_M0_NOP
#define EMI_M0_NOP ""
#else
#define EMI_M0_NOP "s_nop 0\n\t"
#endif

// defect GEMM tile (fp64 MFMA path)
#define DEF_TM 96
#define DEF_TN 128
#define DEF_BK 16

// even/odd defect kernel (emi_symdefect.hip): 16 instances x 64*CT half-indices per workgroup, K tile 16
#define FUSED_TI 16
#define FUSED_BK 16

#include "emi_models.hpp"
#include "emi_pass_work.hpp"

namespace emi {

template <typename T> struct NodeArgs {
    const T* X;         // [B][ns][M]
    const T* U;         // [B][nc][M]
    T* RES;             // [B][nres][M]
    T* VALS;            // [B][nvals][M]
    T* cost_part;       // [B][nchunks]
    T* cost;            // [B]
    unsigned* cost_ticket;  // [B] zeroed once; non-null: the node kernel finishes COST itself (no emi_cost_finish_kernel)
    const T* w;         // [M]  LGL weights
    const T* node_t;    // [M]  node times t0 + h (tau+1)
    const T* Ddiag;     // [M]  D_kk
    const T* path;      // [path_sets][np][EMI_PATH_REC]
    const T* track_x;   // [track_sets][ntracks][M]
    const T* track_y;
    int M, B, np, nres, nvals;
    int path_sets, track_sets, ntracks;
    int px, py;
    int store_mode;     // launcher only: cache policy of the result stores (0 plain, 1 write-through sc1, 2 non-temporal)
    int keep;           // launcher only: 1 = VALS holds the model-invariant rows already, take the KEEP instantiation where there is one
    T h, sgn;
    ModelParams<T> P;
};

template <typename T> struct HessArgs {
    const T* X;
    const T* U;
    const T* lamF;      // [B][ns][M]
    const T* lamC;      // [B][np][M]
    T* H;               // [B][nhess][M]
    const T* w;
    const T* node_t;
    const T* path;
    int M, B, np, path_sets, px, py;
    T h, sgn, sigma;
    ModelParams<T> P;
};

// ODE-error residual at the Gauss points between the nodes (emi_ode_resid_kernel): point p = q (M-1) + k is Gauss point q of
// interval k.  Zs rows (instance, state) hold [E x | E' x | D x] (np + np + M columns, row length lds), Zc rows (instance,
// control) hold E u (row length ldc)
template <typename T> struct OdeResidArgs {
    const T* Zs;        // [B*ns][lds]
    const T* Zc;        // [B*nc][ldc]
    const T* tq;        // [5 (M-1)] times t0 + h (s_p + 1) of the points
    const T* scale;     // [M-1]     (tau_{k+1} - tau_k) / 2 * h
    const T* ul;        // [nc] control bounds (device); null: no clip
    const T* uu;
    T* eta;             // [B][ns][M-1]
    int M, B, lds, ldc;
    T h;
    ModelParams<T> P;
};

// ... of a context with delays (emi_ode_resid_delay_kernel): the model's NC inputs are the ncf free controls, then the delayed slots
// in the order of emi_set_delays.  Zs rows hold [E x | E' x | D x | Edel(dt) x | .. | Edel((xh-1) dt) x] (2 np + M + (xh-1) np
// columns), Zc rows (instance, FREE control) hold [E u | Edel(dt) u | .. | Edel(uh dt) u] ((1 + uh) np columns); np = 5 (M-1)
template <typename T> struct OdeResidDelayArgs {
    const T* Zs;        // [B*ns][lds]
    const T* Zc;        // [B*ncf][ldc]
    const T* tq;
    const T* scale;
    const T* ul;        // [ncf] bounds of the free controls (a delayed copy is clipped with its source's); null: no clip
    const T* uu;
    T* eta;             // [B][ns][M-1]
    int M, B, lds, ldc;
    int ncf, ns, xh, uh;
    T h;
    ModelParams<T> P;
};

// An argument block with a per-instance parameter table behind it (emi_set_model_params_batch): what the TABLED instantiations of the
// node, Hessian and ODE-residual kernels take.  tab [B][EMI_MAX_PARAMS], in the context's real type, already at the launch's first
// instance; the workgroup of instance blockIdx.y reads row blockIdx.y in place of a.P, which it ignores.  The blocks themselves, and
// so what the untabled instantiations read, are as they were.
template <class A, typename T> struct Tabled {
    A a;
    const T* tab;
};

struct SymDefectArgs {
    const double* X;
    const double* U;
    double* RES;
    const double* node_t;
    const double* De;       // [M/2][M/2]  (D[i][j] + D[i][N-j]) / 2
    const double* Do;       // [M/2][M/2]  (D[i][j] - D[i][N-j]) / 2
    int M, B, nres;
    int order;              // block -> tile order within an XCD (see emi_symdefect.hip)
    int ablate;             // diagnostics (results invalid): 4 skip epilogue, 8 all tiles read the X rows of the first 16 instances,
                            // 16 / 32 the MFMA / node role of the one-launch pass returns at once
                            // (1 skip MFMAs, 2 skip operand DMA: the round-1 ring kernel only)
    int ksplit;             // state-split ring kernel: K slices per tile (1 = none); > 1 goes through `slab`
    double* slab;           // [tiles][ksplit][2 SW][4][256] partial sums of a split-K launch
    unsigned* tile_ticket;  // [tiles] zero before the first launch, self-resetting: the slices of a tile are combined by the
                            // workgroup that draws the tile's last ticket (nullptr: emi_symdefect_combine_kernel does it)
    int mfma_first;         // one-launch pass: 1 the MFMA workgroups of an XCD come first in its share of the grid, 0 evenly interleaved
                            // with the node workgroups
    int cpart, cx;          // tile order of the state-split ring kernel (plan_symdefect): the column tiles are cut into cpart
                            // partitions, one per group of 8 / cpart XCDs, and cx column tiles of an X tile run as neighbours
                            // (cpart = 0: plain order, the column tiles of an X tile as neighbours, X tiles dealt over the XCDs;
                            //  cpart = -G: grouped order, super-blocks of G instance groups per XCD, column blocks of cx: ring_tile_of)
    double h;
    ModelParams<double> P;
    const double* Dfrag;    // De / Do once more, in the order the MFMA role's waves consume them (operator_fragments): read only by the
                            // "De / Do from L2" form of the one-launch pass, nullptr where the context holds none
};

struct DefectArgs {
    const double* X;    // [R][M], R = B*ns
    const double* D;    // [M][M] row-major
    double* RES;        // [B][nres][M]; defect rows are accumulated into
    int R, M, ns, nres;
};
struct DefectArgsF32 {
    const float* X;
    const float* D;
    float* RES;
    int R, M, ns, nres;
};
// ring_tile_of (which tile a workgroup of the state-split ring kernel works on), pass_role_of (the role of a block of the one-launch
// pass) and the work table built from the two: emi_pass_work.hpp
// the whole pass as one launch (emi_pass_f64_kernel): both roles' arguments and how the grid is dealt between them
struct PassArgs {
    SymDefectArgs s;
    NodeArgs<double> n;
    int nm8, nn8;           // MFMA / node workgroups per XCD (counts rounded up to a multiple of 8 ...
    int nm, nn;             // ... the workgroups past these real counts do nothing)
    int nbx;                // node chunks per instance
    const PassWork* work;   // [8][nm8 + nn8] what each block of the grid does (pass_work_build, emi_pass_work.hpp): read-only for the launch
};

}  // namespace emi
