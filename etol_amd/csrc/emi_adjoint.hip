// emi_adjoint.hip -- the adjoint pass (fp64): Lagrangian gradient of B trajectories and a tolerance-free KKT certificate.
//
//   G[b][v][k] = sigma * VALS[costgrad v][k]
//              + sum_i VALS[i*nv+v][k] * lamF[i][k]                         node blocks (entry i == v holds D_kk)
//              + (v < ns ? sum_{j != k} D[j][k] * lamF[v][j] : 0)           off-diagonal part of D^T: the operator
//              + sum over path rows and their partials  VALS[..][k] * lamC[r][k]
//
//   KA  emi_adjoint_transpose_kernel   once per mesh: DT[n][j] = D[j][n], zero on the diagonal, rows padded to an even length; with delays
//                                      also WT[n][s*ldt + j] = W_(s+1)[j][n], the transposed stack of the interpolation operators (diagonal kept)
//   KB  emi_adjoint_op_kernel          operator term: [R = B*ns][M] x [M][M] on v_mfma_f64_16x16x4_f64, plain stores into the state rows of G;
//                                      two tile shapes, by the number of workgroups the batch gives.  The same kernel folds the adjoints
//                                      of the delayed values onto their sources (emi_lagr_grad_total_*): rows (instance, source variable),
//                                      K = the delay indices' node ranges one after the other, the last addition is Gx[source] + product
//   KC  emi_adjoint_node_all_kernel /  node terms, threads along the node index: one thread per (instance, node) with the nv sums in registers,
//       emi_adjoint_node_kernel        or per (instance, variable, node) for small batches; both read every VALS entry exactly once
//                                      (coalesced), sum in the same order and ADD the operator term already in G (state rows)
//   KC' emi_adjoint_add_kernel         large batches: KB runs on a second stream beside KC into a block of its own, this adds it onto the state rows
//                                      (the same last addition as back to back: same bits)
//   KD  emi_kkt_certificate_kernel     one workgroup per instance: six maxima by wave shuffles, then LDS; ordinary vector stores
//
// Two kernels instead of a fused epilogue: the product tiles G as (16 instances x 6 states) x 128 nodes, the node
// terms of one G entry need ns + (path partials) VALS rows of that (instance, node): an epilogue would have every lane walk the VALS rows
// of its four accumulator rows -- the same bytes, but 16 nodes wide per load instead of 256, and with the matrix pipe idle meanwhile.  The
// operator term written and read back is B*ns*M*16 bytes, 10 % of VALS at 6 states and 20 keep-outs.
// No atomics anywhere: every G entry has one writer per kernel, every sum a fixed order, a maximum has no order: bit-reproducible.
#include <hip/hip_runtime.h>

#include "emi_kernels.hpp"

namespace emi {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

// tile shapes of the operator product: 96 x 128 (16 instances of a 6-state model per row tile), K tiles of 16, where that gives every CU
// a workgroup; 48 x 64 with K tiles of 32 below that (a config-4 shard of 128 instances is 64 large tiles on 256 CUs, each walking the
// whole K range alone: 133 us against 277 us for eight times the work)
constexpr int ADJ_CUS = 256;
constexpr double ADJ_INF_BOUND = 1e19;      // |bound| >= this: the bound is absent (INF_BOUND of the NLP iteration)

// grid.z = segment: source matrix blockIdx.z, columns blockIdx.z * ldt .. of the ld_dst long rows of DT
__global__ __launch_bounds__(256) void emi_adjoint_transpose_kernel(const double* __restrict__ D, double* __restrict__ DT, int M, int ldt,
                                                                    int ld_dst, int keep_diag) {
    __shared__ double t[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int j0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    D += (size_t)blockIdx.z * M * M;
    DT += (size_t)blockIdx.z * ldt;
    {
        const int j = j0 + ty, n = n0 + tx;
        t[ty][tx] = (j < M && n < M && (keep_diag || j != n)) ? D[(size_t)j * M + n] : 0.0;
    }
    __syncthreads();
    const int n = n0 + ty, j = j0 + tx;
    if (n < M && j < ldt) DT[(size_t)n * ld_dst + j] = t[tx][ty];     // j == M (padding of an odd M) gets the zero staged above
}

// out[r][n] = sum_j lamF[r][j] * DT[n][j];  r = (instance, state): lamF viewed as [R][M]; G rows (instance * nv + state).
// In general (AdjointOpArgs): row r = (instance, j) of A is found through a row map, the K range is nseg segments of ldt (M padded
// to even) each -- segment s reads the A row a_seg * s further down and columns s * ldt .. of Bop -- and the epilogue either stores
// the product or adds one more row to it (add[r][n] + product, one rounding) before the store.
// FOLD = false compiles the operator term alone (A rows contiguous, one segment, plain stores: nothing of the map is evaluated).
// lane l supplies A[l&15][l>>4], B[l>>4][l&15]; result reg i of lane l is out[(l>>4) + 4i][l&15] (as emi_defect_f64_kernel).
// Edge tiles are padded with zeros (rows beyond R, nodes beyond M, K beyond M); every M >= 2.
template <bool ALIGNED, bool FOLD, int TM, int TN, int BK>
__global__ __launch_bounds__(256, 2) void emi_adjoint_op_kernel(AdjointOpArgs a) {
    constexpr int LDK = BK + 2;
    constexpr int RT = TM / 16, CT = TN / 64;
    constexpr int A_PASS = TM * BK / 2 / 256, B_PASS = TN * BK / 2 / 256;
    static_assert(TM * BK / 2 % 256 == 0 && TN * BK / 2 % 256 == 0, "staging shape");
    __shared__ __attribute__((aligned(16))) double smem[2 * (TM + TN) * LDK];
    double* As = smem;                        // [2][TM][LDK]
    double* Bs = smem + 2 * TM * LDK;         // [2][TN][LDK]

    const int M = a.M, R = a.R, ldt = a.ldt, kend = a.nseg * a.ldt;
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    {   // blocks that share a column panel of DT share blockIdx % 8, i.e. one XCD's L2
        const int xcd = bid & 7, q = nwg >> 3, rr = nwg & 7;
        bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
    }
    const int mtiles = (R + TM - 1) / TM;
    const int ntile = bid / mtiles, mtile = bid - ntile * mtiles;
    const int m0 = mtile * TM, n0 = ntile * TN;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r16 = lane & 15, kq = lane >> 4;

    d4 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = d4{0.0, 0.0, 0.0, 0.0};

    double2 pa[A_PASS], pb[B_PASS];
    long long arow[A_PASS];                   // A row (segment 0) of the tile rows this thread stages; -1 beyond R
#pragma unroll
    for (int p = 0; p < A_PASS; ++p) {
        const int r = m0 + (tid + 256 * p) / (BK / 2);
        if (FOLD) {
            const int inst = r / a.rpi;
            arow[p] = r < R ? (long long)inst * a.a_inst + a.a_row0 + (r - inst * a.rpi) : -1;
        } else {
            arow[p] = r < R ? r : -1;
        }
    }
    auto gload = [&](int k0) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) {
            const int c2 = (tid + 256 * p) % (BK / 2);
            int k = k0 + 2 * c2, seg = 0;
            if (FOLD && a.nseg > 1) {
                seg = k / ldt;
                k -= seg * ldt;
            }
            double2 v = make_double2(0.0, 0.0);
            if (arow[p] >= 0 && (!FOLD || seg < a.nseg)) {
                const double* src = a.A + (size_t)(arow[p] + (FOLD ? (long long)seg * a.a_seg : 0)) * M + k;
                if (ALIGNED) {
                    if (k < M) v = *reinterpret_cast<const double2*>(src);
                } else {
                    if (k < M) v.x = src[0];
                    if (k + 1 < M) v.y = src[1];
                }
            }
            pa[p] = v;
        }
#pragma unroll
        for (int p = 0; p < B_PASS; ++p) {
            const int idx = tid + 256 * p, row = idx / (BK / 2), c2 = idx % (BK / 2);
            const int n = n0 + row, k = k0 + 2 * c2;
            double2 v = make_double2(0.0, 0.0);
            if (n < M && k < kend) v = *reinterpret_cast<const double2*>(a.Bop + (size_t)n * a.ldb + k);   // ldt and ldb are even, segments zero padded
            pb[p] = v;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) {
            const int idx = tid + 256 * p, row = idx / (BK / 2), c2 = idx % (BK / 2);
            *reinterpret_cast<double2*>(As + ((size_t)buf * TM + row) * LDK + 2 * c2) = pa[p];
        }
#pragma unroll
        for (int p = 0; p < B_PASS; ++p) {
            const int idx = tid + 256 * p, row = idx / (BK / 2), c2 = idx % (BK / 2);
            *reinterpret_cast<double2*>(Bs + ((size_t)buf * TN + row) * LDK + 2 * c2) = pb[p];
        }
    };

    const int nkt = (kend + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) gload((kt + 1) * BK);
        const double* Ab = As + (size_t)cur * TM * LDK;
        const double* Bb = Bs + ((size_t)cur * TN + wid * (16 * CT)) * LDK;
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            double af[RT], bf[CT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) af[rt] = Ab[(rt * 16 + r16) * LDK + ks * 4 + kq];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) bf[ct] = Bb[(ct * 16 + r16) * LDK + ks * 4 + kq];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[rt], bf[ct], acc[rt][ct], 0, 0, 0);
        }
        if (kt + 1 < nkt) {
            lstore(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
    }

#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int n = n0 + wid * (16 * CT) + ct * 16 + r16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = m0 + rt * 16 + kq + 4 * i;
                if (r < R && n < M) {
                    const int inst = r / a.rpi, j = r - inst * a.rpi;
                    double g = acc[rt][ct][i];
                    if (FOLD && a.add) g = a.add[((size_t)inst * a.add_inst + a.add_row0 + j) * M + n] + g;
                    a.out[((size_t)inst * a.out_inst + a.out_row0 + j) * M + n] = g;
                }
            }
        }
}

// Node terms.  Summation order of one entry, the same in both kernels below (every step one fma): cost gradient, defect rows
// i = 0 .. ns-1, the px partials of the table rows j = 0 .., their py partials, the traced rows' partials by q then j; then the
// operator term already in G is added (state rows).
//
// Form 1: grid (node chunks, nv, B), one thread per (instance, variable, node): the most threads, for small batches and any model.
__global__ __launch_bounds__(256) void emi_adjoint_node_kernel(AdjointArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.M) return;
    const int v = blockIdx.y, b = blockIdx.z;
    const int M = a.M, ns = a.ns, nv = a.ns + a.nc, npt = a.np_table, npm = a.np_traced, pw = a.pw;
    const double* __restrict__ V = a.VALS + (size_t)b * a.nvals * M + k;
    const double* __restrict__ lf = a.lamF + (size_t)b * ns * M + k;
    const double* __restrict__ lc = a.lamC ? a.lamC + (size_t)b * (npt + npm) * M + k : nullptr;
    const int e_tab = ns * nv, e_tr = e_tab + 2 * npt, e_cost = e_tr + npm * pw;
    double g = a.sigma * V[(size_t)(e_cost + v) * M];
#pragma unroll 4
    for (int i = 0; i < ns; ++i) g = fma(V[(size_t)(i * nv + v) * M], lf[(size_t)i * M], g);
    if (npt > 0 && v == a.px) {
#pragma unroll 4
        for (int j = 0; j < npt; ++j) g = fma(V[(size_t)(e_tab + 2 * j) * M], lc[(size_t)j * M], g);
    }
    if (npt > 0 && v == a.py) {
#pragma unroll 4
        for (int j = 0; j < npt; ++j) g = fma(V[(size_t)(e_tab + 2 * j + 1) * M], lc[(size_t)j * M], g);
    }
    for (int q = 0; q < pw; ++q) {
        if (a.pvars[q] != v) continue;
#pragma unroll 4
        for (int j = 0; j < npm; ++j) g = fma(V[(size_t)(e_tr + j * pw + q) * M], lc[(size_t)(npt + j) * M], g);
    }
    double* o = a.G + ((size_t)b * nv + v) * M + k;
    if (a.add_op && v < ns) g += *o;
    *o = g;
}

// Form 2: grid (node chunks, B), one thread per (instance, node) with the nv sums in registers (model dimensions at compile time):
// NS * NV independent coalesced loads in flight per thread, lamF and lamC read once.  For batches that fill the chip.
template <int NS, int NC>
__global__ __launch_bounds__(256) void emi_adjoint_node_all_kernel(AdjointArgs a) {
    constexpr int NV = NS + NC;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.M) return;
    const int b = blockIdx.y;
    const int M = a.M, npt = a.np_table, npm = a.np_traced, pw = a.pw;
    const double* __restrict__ V = a.VALS + (size_t)b * a.nvals * M + k;
    const double* __restrict__ lfp = a.lamF + (size_t)b * NS * M + k;
    const double* __restrict__ lc = a.lamC ? a.lamC + (size_t)b * (npt + npm) * M + k : nullptr;
    const int e_tab = NS * NV, e_tr = e_tab + 2 * npt, e_cost = e_tr + npm * pw;
    double g[NV], lf[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) lf[i] = lfp[(size_t)i * M];
#pragma unroll
    for (int v = 0; v < NV; ++v) g[v] = a.sigma * V[(size_t)(e_cost + v) * M];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int v = 0; v < NV; ++v) g[v] = fma(V[(size_t)(i * NV + v) * M], lf[i], g[v]);
    // a sum that continues g[var] for a run-time var: taken out of and put back into the register array by unrolled compares
    auto run = [&](int var, int e0, int estride, int l0, int n) {
        double x = 0.0;
#pragma unroll
        for (int v = 0; v < NV; ++v) x = v == var ? g[v] : x;
#pragma unroll 4
        for (int j = 0; j < n; ++j) x = fma(V[(size_t)(e0 + j * estride) * M], lc[(size_t)(l0 + j) * M], x);
#pragma unroll
        for (int v = 0; v < NV; ++v) g[v] = v == var ? x : g[v];
    };
    if (npt > 0) {
        run(a.px, e_tab, 2, 0, npt);
        run(a.py, e_tab + 1, 2, 0, npt);
    }
    for (int q = 0; q < pw; ++q) run(a.pvars[q], e_tr + q, pw, npt, npm);
    double* o = a.G + (size_t)b * NV * M + k;
#pragma unroll
    for (int v = 0; v < NV; ++v) o[(size_t)v * M] = (a.add_op && v < NS) ? g[v] + o[(size_t)v * M] : g[v];
}

// side-by-side form: G[b][v < ns][k] = node terms + operator term, the same last addition as in the node kernels
__global__ __launch_bounds__(256) void emi_adjoint_add_kernel(const double* __restrict__ Gop, double* __restrict__ G, int ns, int nv, int M) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    const int v = blockIdx.y, b = blockIdx.z;
    double* o = G + ((size_t)b * nv + v) * M + k;
    *o = *o + Gop[((size_t)b * ns + v) * M + k];
}

__device__ __forceinline__ double adj_max(double x, double y) { return (x > y || x != x) ? x : y; }     // a NaN on either side stays (as numpy's max)

// One workgroup per instance.  cert[b] = {stat, comp, defect, viol, gmax, lmax} (include/emi355x.h).
__global__ __launch_bounds__(256) void emi_kkt_certificate_kernel(CertArgs a) {
    const int b = blockIdx.x, M = a.M, ns = a.ns, nv = a.ns + a.nc, np = a.np;
    const int tid = threadIdx.x;
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double* __restrict__ G = a.G + (size_t)b * nv * M;
    const double* __restrict__ R = a.RES + (size_t)b * a.nres * M;
    const double* __restrict__ cg = a.VALS + ((size_t)b * a.nvals + (a.nvals - a.ncg)) * M;
    const double* __restrict__ zl = a.zl + (a.nsets > 1 ? (size_t)b * nv * M : 0);
    const double* __restrict__ zu = a.zu + (a.nsets > 1 ? (size_t)b * nv * M : 0);
    for (int e = tid; e < nv * M; e += 256) {
        const int v = e / M, k = e - v * M;
        const double g = G[e], gp = adj_max(g, 0.0), gm = adj_max(-g, 0.0);
        const double z = v < ns ? a.X[((size_t)b * ns + v) * M + k] : a.U[((size_t)b * a.nc + (v - ns)) * M + k];
        const double lo = zl[e], up = zu[e];
        const bool has_lo = fabs(lo) < ADJ_INF_BOUND, has_up = fabs(up) < ADJ_INF_BOUND;
        const bool fixed = has_lo && has_up && lo == up;
        if (!fixed) {
            if (has_lo) m[1] = adj_max(m[1], gp * adj_max(z - lo, 0.0)); else m[0] = adj_max(m[0], gp);
            if (has_up) m[1] = adj_max(m[1], gm * adj_max(up - z, 0.0)); else m[0] = adj_max(m[0], gm);
        }
        if (has_lo) m[3] = adj_max(m[3], lo - z);
        if (has_up) m[3] = adj_max(m[3], z - up);
        m[4] = adj_max(m[4], fabs(a.sigma * cg[e]));
    }
    for (int e = nv * M + tid; e < a.ncg * M; e += 256) m[4] = adj_max(m[4], fabs(a.sigma * cg[e]));     // delayed inputs: gmax alone
    for (int e = tid; e < ns * M; e += 256) {
        m[2] = adj_max(m[2], fabs(R[e]));
        m[5] = adj_max(m[5], fabs(a.lamF[(size_t)b * ns * M + e]));
    }
    for (int e = tid; e < np * M; e += 256) {
        const int j = e / M;
        const double c = R[(size_t)ns * M + e], l = a.lamC[(size_t)b * np * M + e];
        const double lp = adj_max(l, 0.0), lm = adj_max(-l, 0.0);
        const double lo = a.cl[j], up = a.cu[j];
        const bool has_lo = fabs(lo) < ADJ_INF_BOUND, has_up = fabs(up) < ADJ_INF_BOUND;
        m[1] = adj_max(m[1], has_up ? lp * adj_max(up - c, 0.0) : lp);
        m[1] = adj_max(m[1], has_lo ? lm * adj_max(c - lo, 0.0) : lm);
        if (has_lo) m[3] = adj_max(m[3], lo - c);
        if (has_up) m[3] = adj_max(m[3], c - up);
        m[5] = adj_max(m[5], fabs(l));
    }
    __shared__ double red[4][6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        double x = m[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x = adj_max(x, __shfl_down(x, off, 64));
        if ((tid & 63) == 0) red[tid >> 6][q] = x;
    }
    __syncthreads();
    if (tid < 6) a.cert[(size_t)b * 6 + tid] = adj_max(adj_max(red[0][tid], red[1][tid]), adj_max(red[2][tid], red[3][tid]));
}

}  // namespace

hipError_t launch_adjoint_transpose(const double* dSrc, double* dDst, int M, int ldt, int ld_dst, int nseg, bool keep_diag, hipStream_t s) {
    dim3 grid((ldt + 15) / 16, (ldt + 15) / 16, nseg);
    hipLaunchKernelGGL(emi_adjoint_transpose_kernel, grid, dim3(256), 0, s, dSrc, dDst, M, ldt, ld_dst, keep_diag ? 1 : 0);
    return hipGetLastError();
}

// node terms of the instances [b0, b0 + nb): form 2 where the model has an instantiation and the batch fills the chip, else form 1
static bool launch_adjoint_node_rows(const AdjointArgs& a, hipStream_t s, hipError_t* err) {
    const int nv = a.ns + a.nc, chunks = (a.M + 255) / 256;
    const bool all_form = (long long)a.B * chunks >= 2 * ADJ_CUS &&
                          ((a.ns == 2 && a.nc == 2) || (a.ns == 6 && a.nc == 2) || (a.ns == 12 && a.nc == 4));
    for (int b0 = 0; b0 < a.B; b0 += 65535) {          // grid.y / grid.z carry at most 65535 instances per launch
        AdjointArgs p = a;
        const int nb = a.B - b0 < 65535 ? a.B - b0 : 65535;
        p.B = nb;
        p.VALS = a.VALS + (size_t)b0 * a.nvals * a.M;
        p.lamF = a.lamF + (size_t)b0 * a.ns * a.M;
        p.lamC = a.lamC ? a.lamC + (size_t)b0 * (a.np_table + a.np_traced) * a.M : nullptr;
        p.G = a.G + (size_t)b0 * nv * a.M;
        if (!all_form) hipLaunchKernelGGL(emi_adjoint_node_kernel, dim3(chunks, nv, nb), dim3(256), 0, s, p);
        else if (a.ns == 2) hipLaunchKernelGGL((emi_adjoint_node_all_kernel<2, 2>), dim3(chunks, nb), dim3(256), 0, s, p);
        else if (a.ns == 6) hipLaunchKernelGGL((emi_adjoint_node_all_kernel<6, 2>), dim3(chunks, nb), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((emi_adjoint_node_all_kernel<12, 4>), dim3(chunks, nb), dim3(256), 0, s, p);
        if ((*err = hipGetLastError()) != hipSuccess) return true;
    }
    return false;
}

// the batch gives the large tile shape a workgroup per CU: the product is then long enough to run beside the node kernel
bool adjoint_side_by_side(int B, int ns, int M) { return ((B * ns + 95) / 96) * ((M + 127) / 128) >= ADJ_CUS; }

hipError_t launch_adjoint_op(const AdjointArgs& a, hipStream_t s) {
    AdjointOpArgs o;
    o.A = a.lamF; o.Bop = a.DT; o.add = nullptr; o.out = a.G;
    o.R = a.B * a.ns; o.rpi = a.ns; o.M = a.M; o.ldt = a.ldt; o.nseg = 1; o.ldb = a.ldt;
    o.a_inst = a.ns; o.a_row0 = 0; o.a_seg = 0; o.out_inst = a.ns + a.nc; o.out_row0 = 0; o.add_inst = 0; o.add_row0 = 0;
    return launch_adjoint_product(o, 0, s);
}

hipError_t launch_adjoint_product(const AdjointOpArgs& a, int tile, hipStream_t s) {
    const int R = a.R;
    const int big = ((R + 95) / 96) * ((a.M + 127) / 128), small = ((R + 47) / 48) * ((a.M + 63) / 64);
    const bool al = a.M % 2 == 0;
    // the operator term: rows of A one after the other, one segment, plain stores
    const bool fold = a.nseg != 1 || a.add || a.a_row0 != 0 || a.a_inst != a.rpi;
    const bool large = tile == 2 || (tile == 0 && big >= ADJ_CUS);
#define EMI_ADJ_LAUNCH(AL, FO)                                                                                                      \
    do {                                                                                                                            \
        if (large) hipLaunchKernelGGL((emi_adjoint_op_kernel<AL, FO, 96, 128, 16>), dim3(big), dim3(256), 0, s, a);                 \
        else hipLaunchKernelGGL((emi_adjoint_op_kernel<AL, FO, 48, 64, 32>), dim3(small), dim3(256), 0, s, a);                      \
    } while (0)
    if (fold) {
        if (al) EMI_ADJ_LAUNCH(true, true);
        else EMI_ADJ_LAUNCH(false, true);
    } else {
        if (al) EMI_ADJ_LAUNCH(true, false);
        else EMI_ADJ_LAUNCH(false, false);
    }
#undef EMI_ADJ_LAUNCH
    return hipGetLastError();
}

hipError_t launch_adjoint_nodes(const AdjointArgs& a, hipStream_t s) {
    hipError_t e = hipSuccess;
    launch_adjoint_node_rows(a, s, &e);
    return e;
}

hipError_t launch_adjoint_add(const double* dGop, double* dG, int B, int ns, int nv, int M, hipStream_t s) {
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        hipLaunchKernelGGL(emi_adjoint_add_kernel, dim3((M + 255) / 256, ns, nb), dim3(256), 0, s, dGop + (size_t)b0 * ns * M,
                           dG + (size_t)b0 * nv * M, ns, nv, M);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_kkt_certificate(const CertArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(emi_kkt_certificate_kernel, dim3(a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace emi
