// emi_kkt_blocks.hip -- the node blocks of the Newton step, assembled and made positive definite on the device (fp64, gfx950).
//
// What the host loop of solve_nlp does once per factorisation attempt (host/emi_nlp.cpp: assemble_node_blocks and
// convexify_node_blocks), over [instance][node]:
//     Q_k = H_k + Sigma_k + dw_shift (free diagonals) + sum_j sig_t,j g_j g_j^T
// then, per block: identity rows for fixed variables, diagonal scaling d_v = sqrt(max(|A_vv|, 1e-12 amax)), a Cholesky screen
// (pivot <= 10 fl fails, fl = 1e-9) and, for a block that fails, a Jacobi eigen-decomposition of the scaled block with negative
// eigenvalues reflected and recorded (what emi_kkt_lowrank takes).  Four launches, no atomics, every sum in a fixed order:
//
//   A  emi_blocks_assemble_kernel   one thread per (instance, node), the packed triangle in registers; writes Qexact and Q,
//                                   runs scaling + screen in place and writes a flag per node.  Every access is along the node axis.
//   -  emi_blocks_compact_kernel    one workgroup per instance: the flagged nodes in ascending order (ballot prefix scan)
//   B  emi_blocks_eigfix_kernel     one group of NVP lanes (NVP = 4, 8, 16 >= nv) per flagged block; lane r owns row r of the
//                                   scaled block and of the eigenvector matrix, in registers.  Round-robin Jacobi: NVP - 1 steps per
//                                   sweep, NVP / 2 disjoint rotations per step; rows meet through lane shuffles (no LDS, no scratch).
//   C  emi_blocks_list_kernel       one workgroup per instance: offsets of the recorded pairs by a prefix scan over the flagged
//                                   nodes, the list (node, delta, vec) up to max_mods entries, the TRUE count, and worst.
#include <hip/hip_runtime.h>

#include "emi_kernels.hpp"

namespace emi {
namespace {

constexpr double BLK_FL = 1e-9;      // eigenvalue floor / screen threshold of the scaled block (convexify_node_blocks)

__host__ __device__ constexpr int tri(int v, int q) { return v * (v + 1) / 2 + q; }      // packed lower triangle, q <= v

// ---- stage A ------------------------------------------------------------------------------------------------------------------
// NV: block size the loops are unrolled to; GEN: the block size is a.nv <= NV (rows beyond it are an identity that takes no part)
template <int NV, bool GEN>
__global__ __launch_bounds__(64) void emi_blocks_assemble_kernel(BlocksArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (k >= a.M) return;
    const int nv = GEN ? a.nv : NV, nh = nv * (nv + 1) / 2;
    const size_t M = (size_t)a.M;
    const double* H = a.H + (size_t)b * nh * M + k;
    const double* V = a.VALS + (size_t)b * a.nvals * M + k;
    const double* Sg = a.Sigma + (size_t)b * nv * M + k;
    const double* St = a.SigT + (size_t)b * a.np * M + k;       // (not read when there are no terms)
    const unsigned char* fx = a.fixed + (size_t)b * nv * M + k;
    double* Qx = a.Qexact ? a.Qexact + (size_t)b * nh * M + k : nullptr;
    double* Qo = a.Q + (size_t)b * nh * M + k;

    unsigned fxm = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v)
        if (!GEN || v < nv) fxm |= fx[v * M] ? 1u << v : 0u;

    // assembly, entry by entry: H, then Sigma + dw_shift on a free diagonal, then the path-row terms of this entry in row order
    double q[NV * (NV + 1) / 2];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int c = 0; c <= v; ++c) {
            const int e = tri(v, c);
            if (GEN && v >= nv) { q[e] = v == c ? 1.0 : 0.0; continue; }
            double acc = H[e * M];
            if (v == c) acc += Sg[v * M] + ((fxm >> v & 1u) ? 0.0 : a.dw_shift);
            for (int t = a.term_ptr[e]; t < a.term_ptr[e + 1]; ++t)
                acc += St[a.term_row[t] * M] * V[a.term_ea[t] * M] * V[a.term_eb[t] * M];
            if (Qx) Qx[e * M] = acc;
            Qo[e * M] = acc;
            q[e] = acc;
        }

    // the working block: identity rows and columns for fixed variables
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int c = 0; c <= v; ++c)
            if ((fxm >> v & 1u) || (fxm >> c & 1u)) q[tri(v, c)] = v == c ? 1.0 : 0.0;
    double amax = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int c = 0; c <= v; ++c)
            if (!GEN || v < nv) amax = fmax(amax, fabs(q[tri(v, c)]));
    if (amax == 0.0) amax = 1.0;
    double d[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) d[v] = (!GEN || v < nv) ? sqrt(fmax(fabs(q[tri(v, v)]), 1e-12 * amax)) : 1.0;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int c = 0; c <= v; ++c) q[tri(v, c)] /= d[v] * d[c];
    // Cholesky screen, in place, row by row (the verdict is the first failing pivot's; what follows it is not used)
    bool pd = true;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double sum = q[tri(i, j)];
#pragma unroll
            for (int t = 0; t < j; ++t) sum -= q[tri(i, t)] * q[tri(j, t)];
            if (i == j) {
                if (!(sum > 10.0 * BLK_FL)) { pd = false; sum = 1.0; }
                q[tri(i, i)] = sqrt(sum);
            } else {
                q[tri(i, j)] = sum / q[tri(j, j)];
            }
        }
    a.flag[(size_t)b * M + k] = pd ? 0 : 1;
}

// ---- flagged nodes of every instance, ascending ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emi_blocks_compact_kernel(const int* flag, int* list, int* nflag, int M) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int base = 0;
    for (int k0 = 0; k0 < M; k0 += 256) {
        const int k = k0 + tid;
        const int f = k < M ? flag[(size_t)b * M + k] : 0;
        const unsigned long long bal = __ballot(f != 0);
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
        for (int i = 0; i < 4; ++i) {
            if (i < w) off += wsum[i];
            tot += wsum[i];
        }
        if (f) list[(size_t)b * M + off + __popcll(bal & ((1ull << lane) - 1ull))] = k;
        base += tot;
        __syncthreads();
    }
    if (tid == 0) nflag[b] = base;
}

// ---- stage B ------------------------------------------------------------------------------------------------------------------
// Round-robin pairing (circle method) in its systolic form: the pairs of every step are the slots (0,1), (2,3), ..; between
// steps the rows and columns move: slot 0 stays, the others walk a cycle of length N - 1 (even slots upwards, odd slots
// downwards).  Every two indices meet exactly once in N - 1 steps, after which every index is back in its own slot -- so the
// steps of a sweep are one body in a loop, with constant register indices.  rr_src(N, j): the slot whose content moves to slot j.
__host__ __device__ constexpr int rr_src(int N, int j) {
    return j == 0 ? 0 : j == 2 ? 1 : j % 2 == 0 ? j - 2 : j == N - 1 ? N - 2 : j + 2;
}

template <int NVP>
__device__ __forceinline__ double group_sum(double x) {
#pragma unroll
    for (int m = 1; m < NVP; m <<= 1) x += __shfl_xor(x, m, NVP);
    return x;
}
template <int NVP>
__device__ __forceinline__ double group_max(double x) {
#pragma unroll
    for (int m = 1; m < NVP; m <<= 1) x = fmax(x, __shfl_xor(x, m, NVP));
    return x;
}

// One step of a sweep: the NVP / 2 rotations of the slots (2i, 2i + 1), then the move to the next pairing.
// A: row r of the block with its own diagonal kept in dd (slot r holds 0); V: row r of the eigenvector matrix (its COLUMNS move
// with the slots, its rows stay with their lanes).
template <int NVP>
__device__ __forceinline__ void jacobi_step(double (&A)[NVP], double (&V)[NVP], double& dd, int r, bool done) {
    const int partner = r ^ 1, lo = r & ~1, mine = r >> 1;
    const bool is_lo = (r & 1) == 0;
    double apq = 0.0;
#pragma unroll
    for (int j = 0; j < NVP; ++j)
        if (j == partner) apq = A[j];
    // both lanes of a pair rotate by the lower lane's copy of the off-diagonal entry: the same angle in both
    apq = __shfl(apq, lo, NVP);
    const double app = __shfl(dd, lo, NVP), aqq = __shfl(dd, lo + 1, NVP);
    double c = 1.0, sn = 0.0, t = 0.0;
    if (apq != 0.0 && !done) {
        const double theta = (aqq - app) / (2.0 * apq);
        t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        c = 1.0 / sqrt(t * t + 1.0);
        sn = t * c;
    }
    // columns: every lane applies every rotation of the step to its row (its own pair's two entries are set below)
#pragma unroll
    for (int i = 0; i < NVP / 2; ++i) {
        const double ci = __shfl(c, 2 * i, NVP), si = __shfl(sn, 2 * i, NVP);
        const double vp = V[2 * i], vq = V[2 * i + 1];
        V[2 * i] = ci * vp - si * vq;
        V[2 * i + 1] = si * vp + ci * vq;
        if (i != mine) {
            const double ap = A[2 * i], aq = A[2 * i + 1];
            A[2 * i] = ci * ap - si * aq;
            A[2 * i + 1] = si * ap + ci * aq;
        }
    }
    // rows: the two lanes of a pair combine their rows; the rotated entry becomes 0 (as does the unused diagonal slot)
#pragma unroll
    for (int j = 0; j < NVP; ++j) {
        const double pj = __shfl(A[j], partner, NVP);
        A[j] = (j >> 1) == mine ? 0.0 : is_lo ? c * A[j] - sn * pj : sn * pj + c * A[j];
    }
    dd = is_lo ? dd - t * apq : dd + t * apq;
    // the move: columns by renaming, rows from the lane that held them
    const int from = rr_src(NVP, r);
    double An[NVP], Vn[NVP];
#pragma unroll
    for (int j = 0; j < NVP; ++j) { An[j] = A[rr_src(NVP, j)]; Vn[j] = V[rr_src(NVP, j)]; }
#pragma unroll
    for (int j = 0; j < NVP; ++j) { A[j] = __shfl(An[j], from, NVP); V[j] = Vn[j]; }
    dd = __shfl(dd, from, NVP);
}

template <int NVP>
__global__ __launch_bounds__(64) void emi_blocks_eigfix_kernel(BlocksArgs a) {
    constexpr int G = 64 / NVP;
    const int b = blockIdx.y, nf = a.nflag[b];
    if ((int)blockIdx.x * G >= nf) return;                    // (the whole workgroup)
    const int lane = threadIdx.x, r = lane % NVP, f = blockIdx.x * G + lane / NVP;
    const bool act = f < nf;                                    // a group without a block carries an identity and stores nothing
    const int nv = a.nv, nh = nv * (nv + 1) / 2;
    const size_t M = (size_t)a.M;
    const int k = act ? a.list[(size_t)b * M + f] : 0;
    const bool row = act && r < nv;
    const bool fxr = row && a.fixed[((size_t)b * nv + r) * M + k] != 0;
    double* Qo = a.Q + (size_t)b * nh * M + k;

    unsigned fxm = 0;
#pragma unroll
    for (int j = 0; j < NVP; ++j) fxm |= __shfl((int)fxr, j, NVP) ? 1u << j : 0u;
    double A[NVP], V[NVP];
    double amax = 0.0, diag = 1.0;
#pragma unroll
    for (int j = 0; j < NVP; ++j) {
        double x = r == j ? 1.0 : 0.0;
        const bool in = row && j < nv;
        if (in && !fxr && !(fxm >> j & 1u)) x = Qo[(size_t)(r > j ? tri(r, j) : tri(j, r)) * M];
        if (in) amax = fmax(amax, fabs(x));
        if (j == r) diag = x;
        A[j] = x;
        V[j] = r == j ? 1.0 : 0.0;
    }
    amax = group_max<NVP>(amax);
    if (amax == 0.0) amax = 1.0;
    const double dr = row ? sqrt(fmax(fabs(diag), 1e-12 * amax)) : 1.0;
#pragma unroll
    for (int j = 0; j < NVP; ++j) A[j] /= dr * __shfl(dr, j, NVP);
    double dd = diag / (dr * dr);
#pragma unroll
    for (int j = 0; j < NVP; ++j)
        if (j == r) A[j] = 0.0;

    bool done = false;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int j = 0; j < NVP; ++j) off += A[j] * A[j];                // both copies of every off-diagonal entry
        off = 0.5 * group_sum<NVP>(off);
        const double dia = group_sum<NVP>(dd * dd);
        if (off < 1e-32 * fmax(1.0, dia)) done = true;
        if (!__any(!done)) break;
#pragma unroll 1
        for (int step = 0; step < NVP - 1; ++step) jacobi_step<NVP>(A, V, dd, r, done);
    }

    // the host's rules: nl = max(|lambda|, fl); lambda < -fl is recorded (delta = nl - lambda, v = d o eigenvector), the pairs of a
    // node in ascending eigenvalue order; Q~ = d o (V diag(nl) V^T) o d on the entries whose two variables are free
    const double lam = dd, nl = fmax(fabs(lam), BLK_FL);
    const bool neg = row && lam < -BLK_FL;
    int rank = 0, cnt = 0;
#pragma unroll
    for (int j = 0; j < NVP; ++j) {
        const double lj = __shfl(lam, j, NVP);
        if (__shfl((int)neg, j, NVP)) {
            ++cnt;
            if (lj < lam || (lj == lam && j < r)) ++rank;
        }
    }
    const double d0 = __shfl(dr, 0, NVP);
    const size_t blk = (size_t)b * M + f;
    const double worst = group_max<NVP>(neg ? (nl - lam) * d0 * d0 : 0.0);
    if (neg) a.tdelta[blk * nv + rank] = nl - lam;
    if (act && r == 0) { a.tworst[blk] = worst; a.cnt[blk] = cnt; }
#pragma unroll
    for (int i = 0; i < NVP; ++i) {
        const int ri = __shfl(rank, i, NVP);
        if (__shfl((int)neg, i, NVP) && row) a.tvec[(blk * nv + ri) * nv + r] = dr * V[i];
    }
    double W[NVP];
#pragma unroll
    for (int e = 0; e < NVP; ++e) W[e] = V[e] * __shfl(nl, e, NVP);
#pragma unroll 1
    for (int c = 0; c < NVP; ++c) {                           // (row c of V comes by shuffle from lane c: no register is indexed by c)
        double sum = 0.0;
#pragma unroll
        for (int e = 0; e < NVP; ++e) sum += W[e] * __shfl(V[e], c, NVP);
        const double dc = __shfl(dr, c, NVP);
        if (row && c <= r && !fxr && !(fxm >> c & 1u)) Qo[(size_t)tri(r, c) * M] = dr * dc * sum;
    }
}

// ---- stage C ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emi_blocks_list_kernel(BlocksArgs a) {
    __shared__ int wsum[4];
    __shared__ double wmax[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nf = a.nflag[b], nv = a.nv, mm = a.max_mods;
    const size_t M = (size_t)a.M;
    int base = 0;
    double worst = 0.0;
    for (int f0 = 0; f0 < nf; f0 += 256) {
        const int f = f0 + tid;
        const size_t blk = (size_t)b * M + f;
        const int c = f < nf ? a.cnt[blk] : 0;
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int off = base + incl - c, tot = 0;
        for (int i = 0; i < 4; ++i) {
            if (i < w) off += wsum[i];
            tot += wsum[i];
        }
        if (c > 0) {
            const int k = a.list[blk];
            for (int i = 0; i < c; ++i) {
                const int idx = off + i;
                if (idx >= mm) break;
                const size_t o = (size_t)b * mm + idx;
                a.node[o] = k;
                a.delta[o] = a.tdelta[blk * nv + i];
                for (int v = 0; v < nv; ++v) a.vec[o * nv + v] = a.tvec[(blk * nv + i) * nv + v];
            }
            worst = fmax(worst, a.tworst[blk]);
        }
        base += tot;
        __syncthreads();
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) worst = fmax(worst, __shfl_xor(worst, m));
    if (lane == 0) wmax[w] = worst;
    __syncthreads();
    if (tid == 0) {
        a.count[b] = base;
        a.worst[b] = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    }
}

}  // namespace

hipError_t launch_kkt_blocks(const BlocksArgs& a, hipStream_t s) {
    const dim3 grid_a((a.M + 63) / 64, a.B), blk64(64);
    if (!a.generic && a.nv == 4) hipLaunchKernelGGL((emi_blocks_assemble_kernel<4, false>), grid_a, blk64, 0, s, a);
    else if (!a.generic && a.nv == 8) hipLaunchKernelGGL((emi_blocks_assemble_kernel<8, false>), grid_a, blk64, 0, s, a);
    else if (!a.generic && a.nv == 16) hipLaunchKernelGGL((emi_blocks_assemble_kernel<16, false>), grid_a, blk64, 0, s, a);
    else hipLaunchKernelGGL((emi_blocks_assemble_kernel<16, true>), grid_a, blk64, 0, s, a);
    hipLaunchKernelGGL(emi_blocks_compact_kernel, dim3(a.B), dim3(256), 0, s, a.flag, a.list, a.nflag, a.M);
    // a lane group per flagged block; the grid covers every node, a workgroup beyond the flagged ones returns at once
    if (a.nv <= 4) hipLaunchKernelGGL(emi_blocks_eigfix_kernel<4>, dim3((a.M + 15) / 16, a.B), blk64, 0, s, a);
    else if (a.nv <= 8) hipLaunchKernelGGL(emi_blocks_eigfix_kernel<8>, dim3((a.M + 7) / 8, a.B), blk64, 0, s, a);
    else hipLaunchKernelGGL(emi_blocks_eigfix_kernel<16>, dim3((a.M + 3) / 4, a.B), blk64, 0, s, a);
    hipLaunchKernelGGL(emi_blocks_list_kernel, dim3(a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace emi
