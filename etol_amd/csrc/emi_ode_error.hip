// emi_ode_error.hip -- the relative local ODE error of B trajectories on the context's collocation mesh (fp64; the definition:
// include/emi355x.h, emi_ode_error_*).
//
//   KA  emi_ode_copy_D_kernel     once per mesh: the D block of the stacked operator [E | E' | D], rows padded to an even length
//                                 (E and E' come from the host, emi_ode_error_operator)
//   KB  emi_interp_op_kernel      out[r][c] = sum_j V[r][j] OP[c][j] on v_mfma_f64_16x16x4_f64: state rows against the stacked
//                                 operator (x~, h x~', D x from one launch), control rows against E alone; two tile shapes, by the
//                                 number of workgroups the launch gives
//   KC  emi_ode_resid_kernel      (emi_node_kernels.hpp, per model) one thread per (instance, interval): f at the five Gauss
//                                 points, eta[b][i][k]
//   KD  emi_ode_finish_kernel     one workgroup per instance: the state scales W[b][i], then err[b] = max eta / (W + 1), by wave
//                                 shuffles and then LDS in wave order; ordinary vector stores
//
// Three kernels instead of an epilogue on the product: f at a point needs every variable of that (instance,
// point), the product's accumulators hold 4 rows x 1 column per lane.  No atomics, no split-K: every output has one writer and
// every sum a fixed order, a maximum has no order: bit-reproducible, and a row's bits depend on that row and the operator alone.
#include <hip/hip_runtime.h>

#include "emi_kernels.hpp"

namespace emi {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int ODE_CUS = 256;

__global__ __launch_bounds__(256) void emi_ode_copy_D_kernel(const double* __restrict__ D, double* __restrict__ dst, int M, int ldk) {
    const int j = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (j < ldk) dst[(size_t)k * ldk + j] = j < M ? D[(size_t)k * M + j] : 0.0;
}

// Fragment layout and edge tiles as emi_adjoint_op_kernel (emi_adjoint.hip), whose output has N = M wired in: lane l supplies
// V[l&15][l>>4], OP[l&15][l>>4] of a 16 x 4 step; result reg i of lane l is out[(l>>4) + 4i][l&15].  Edge tiles are padded with
// zeros (rows beyond R, columns beyond N, K beyond the row length), which adds exact zeros: the bits of an output do not depend
// on the tile shape.  Any R >= 1, K >= 2, N >= 1.
template <bool ALIGNED, int TM, int TN, int BK>
__global__ __launch_bounds__(256, 2) void emi_interp_op_kernel(InterpOpArgs a) {
    constexpr int LDK = BK + 2;
    constexpr int RT = TM / 16, CT = TN / 64;
    constexpr int A_PASS = TM * BK / 2 / 256, B_PASS = TN * BK / 2 / 256;
    static_assert(TM * BK / 2 % 256 == 0 && TN * BK / 2 % 256 == 0, "staging shape");
    __shared__ __attribute__((aligned(16))) double smem[2 * (TM + TN) * LDK];
    double* As = smem;                        // [2][TM][LDK]
    double* Bs = smem + 2 * TM * LDK;         // [2][TN][LDK]

    const int K = a.K, R = a.R, N = a.N, ldk = a.ldk;
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    {   // blocks that share a column panel of OP share blockIdx % 8, i.e. one XCD's L2
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
    auto gload = [&](int k0) {
#pragma unroll
        for (int p = 0; p < A_PASS; ++p) {
            const int idx = tid + 256 * p, r = m0 + idx / (BK / 2), k = k0 + 2 * (idx % (BK / 2));
            double2 v = make_double2(0.0, 0.0);
            if (r < R) {
                const double* src = a.V + (size_t)r * K + k;
                if (ALIGNED) {
                    if (k < K) v = *reinterpret_cast<const double2*>(src);
                } else {
                    if (k < K) v.x = src[0];
                    if (k + 1 < K) v.y = src[1];
                }
            }
            pa[p] = v;
        }
#pragma unroll
        for (int p = 0; p < B_PASS; ++p) {
            const int idx = tid + 256 * p, n = n0 + idx / (BK / 2), k = k0 + 2 * (idx % (BK / 2));
            double2 v = make_double2(0.0, 0.0);
            if (n < N && k < ldk) v = *reinterpret_cast<const double2*>(a.OP + (size_t)n * ldk + k);   // ldk is even, rows zero padded
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

    const int nkt = (ldk + BK - 1) / BK;
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
                if (r < R && n < N) a.out[(size_t)r * a.ldo + n] = acc[rt][ct][i];
            }
        }
}

__device__ __forceinline__ double ode_max(double x, double y) { return (x > y || x != x) ? x : y; }     // a NaN on either side stays

// the maximum of x over the workgroup, in every thread: wave shuffles, then LDS in wave order
__device__ __forceinline__ double ode_block_max(double x, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = ode_max(x, __shfl_down(x, off, 64));
    __syncthreads();                // (the previous round's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ode_max(ode_max(red[0], red[1]), ode_max(red[2], red[3]));
}

// One workgroup per instance.  W[i] = max_k max(|x_ik|, |(D x)_ik| / h);  err = max_{i,k} eta[i][k] / (W[i] + 1).
__global__ __launch_bounds__(256) void emi_ode_finish_kernel(OdeFinishArgs a) {
    const int b = blockIdx.x, M = a.M, ns = a.ns, nq = M - 1, tid = threadIdx.x;
    __shared__ double red[4];
    double e = 0.0;
    for (int i = 0; i < ns; ++i) {
        const double* __restrict__ x = a.X + ((size_t)b * ns + i) * M;
        const double* __restrict__ dx = a.Zs + ((size_t)b * ns + i) * a.lds + a.dcol;
        const double* __restrict__ eta = a.eta + ((size_t)b * ns + i) * nq;
        double w = 0.0;
        for (int k = tid; k < M; k += 256) w = ode_max(w, ode_max(fabs(x[k]), fabs(dx[k]) / a.h));
        w = ode_block_max(w, red);
        for (int k = tid; k < nq; k += 256) e = ode_max(e, eta[k] / (w + 1.0));
    }
    e = ode_block_max(e, red);
    if (tid == 0) a.err[b] = e;
}

}  // namespace

hipError_t launch_ode_copy_D(const double* D, double* dst, int M, int ldk, hipStream_t s) {
    hipLaunchKernelGGL(emi_ode_copy_D_kernel, dim3((ldk + 255) / 256, M), dim3(256), 0, s, D, dst, M, ldk);
    return hipGetLastError();
}

// tile shapes as the adjoint product's: 96 x 128 with K tiles of 16 where that gives every CU a workgroup, 48 x 64 with K tiles of
// 32 below that
hipError_t launch_interp_op(const InterpOpArgs& a, hipStream_t s) {
    const long long big = (long long)((a.R + 95) / 96) * ((a.N + 127) / 128), small = (long long)((a.R + 47) / 48) * ((a.N + 63) / 64);
    if (small > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool al = a.K % 2 == 0 && ((size_t)a.V & 15) == 0;        // rows of V start on 16 bytes: loaded as pairs
    if (big >= ODE_CUS) {
        if (al) hipLaunchKernelGGL((emi_interp_op_kernel<true, 96, 128, 16>), dim3((unsigned)big), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((emi_interp_op_kernel<false, 96, 128, 16>), dim3((unsigned)big), dim3(256), 0, s, a);
    } else {
        if (al) hipLaunchKernelGGL((emi_interp_op_kernel<true, 48, 64, 32>), dim3((unsigned)small), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((emi_interp_op_kernel<false, 48, 64, 32>), dim3((unsigned)small), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_ode_finish(const OdeFinishArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(emi_ode_finish_kernel, dim3(a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace emi
