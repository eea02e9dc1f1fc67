// mfma_mix_probe.hip -- diagnostic: what does each ingredient of the defect kernel's inner loop cost the fp64 matrix
// pipe?  One "tile" = 24 x v_mfma_f64_16x16x4_f64 (12 accumulators x 2 k-steps), as in emi_symdefect_ring2_f64_kernel.
//   bit 0: the A operands are produced by v_add_f64 / v_sub from two loaded values (e = xf + xm, o = xf - xm)
//   bit 1: the operands of every tile are read from LDS (14 ds_read_b128 per wave and tile)
//   bit 2: one s_barrier per tile (256-thread workgroups)
//   bit 3: 5 LDS-DMA instructions (global_load_lds_dwordx4, 1 KB each) per wave and tile from an L2-resident buffer,
//          counted vmcnt two tiles behind
//   bit 4: (with bit 3) the B operands (De / Do rows, private to a wave) do not go through LDS: two 16-byte global
//          loads per lane and tile straight into registers (inline asm, one tile ahead), 3 LDS-DMA instructions left
// W = workgroups per CU (1 or 2).  Prints cycles per MFMA per SIMD (64 = the pipe's rate) and TFLOP/s.
// Bits 3 and 4 issue their DMA through the builtin, after which the compiler drains vmcnt ahead of every LDS read: they compare two
// drained loops.  The K loop as shipped (inline-assembly DMA, counted vmcnt, software-pipelined, 16 MFMAs per 16-deep tile) with De / Do
// through the ring or straight from L2 is kloop<FORM> below; it runs first (MFMA_MIX_KLOOP_ONLY set: nothing else runs).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double d4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <int MODE>
__global__ __launch_bounds__(256, 2) void tile_loop(int tiles, unsigned long long* stamps, double* sink, const double* gbuf) {
    extern __shared__ __attribute__((aligned(16))) double smem[];      // 3 stages x 20 KB
    constexpr int STAGE = 320 * 8;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r16 = lane & 15, kq = lane >> 4;
    for (int i = tid; i < 3 * STAGE; i += 256) smem[i] = 1.0 + 1e-6 * i;
    __syncthreads();
    d4 acc_a[6], acc_b[6];
    for (int s = 0; s < 6; ++s) { acc_a[s] = d4{0, 0, 0, 0}; acc_b[s] = d4{0, 0, 0, 0}; }
    double2 be = make_double2(1.0 + lane * 1e-3, 0.5), bo = make_double2(0.25, 2.0 - lane * 1e-3);
    double2 xf[6], xm[6];
    for (int s = 0; s < 6; ++s) { xf[s] = make_double2(0.1 * s + lane, 1.0); xm[s] = make_double2(0.3, 0.7 * s); }
    const double* src = gbuf + ((size_t)blockIdx.x * 64 + lane) * 2 + wid * 128;
    auto issue = [&](int stage, int kt) {
#pragma unroll
        for (int t = 0; t < ((MODE & 16) ? 3 : 5); ++t) {
            double* dst = smem + (size_t)stage * STAGE + (size_t)(wid + 4 * t) * 128;
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + ((kt * 5 + t) & 63) * 512), (lds_ptr_t)dst, 16, 0, 0);
        }
    };
    typedef int v4i __attribute__((ext_vector_type(4)));
    v4i dn0 = {0, 0, 0, 0}, dn1 = {0, 0, 0, 0};          // B fragments of the NEXT tile, in flight
    const double* dsrc = gbuf + (size_t)(blockIdx.x & 63) * 4096 + (wid * 16 + r16) * 64 + kq * 2;
    auto dload = [&](int kt) {
        const double* g0 = dsrc + (kt & 7) * 8, *g1 = g0 + 2048;
        asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %3, off" : "=v"(dn0), "=v"(dn1) : "v"(g0), "v"(g1) : "memory");
    };
    if (MODE & 8) { issue(0, 0); if (MODE & 16) dload(0); issue(1, 1); }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int kt = 0; kt < tiles; ++kt) {
        if ((MODE & 24) == 24) {
            // outstanding, oldest first: X(kt) | D(kt) | X(kt+1): all but the 3 youngest must have landed
            asm volatile("s_waitcnt vmcnt(3)" : "+v"(dn0), "+v"(dn1) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_memcpy(&be, &dn0, 16);
            __builtin_memcpy(&bo, &dn1, 16);
        } else if (MODE & 8) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        if (MODE & 4) asm volatile("s_barrier" ::: "memory");
        if ((MODE & 24) == 24) dload(kt + 1);
        if (MODE & 8) issue((kt + 2) % 3, kt + 2);
        if (MODE & 2) {
            const double* S = smem + (size_t)(kt % 3) * STAGE;
            const int rb = wid * 16 + r16;
            if (!(MODE & 16)) {
                be = *reinterpret_cast<const double2*>(S + 192 * 8 + rb * 8 + ((kq ^ ((0 - (rb >> 2)) & 3)) << 1));
                bo = *reinterpret_cast<const double2*>(S + 256 * 8 + rb * 8 + ((kq ^ ((0 - (rb >> 2)) & 3)) << 1));
            }
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const int r = s * 16 + r16;
                xf[s] = *reinterpret_cast<const double2*>(S + r * 8 + ((kq ^ ((0 - (r >> 2)) & 3)) << 1));
                xm[s] = *reinterpret_cast<const double2*>(S + (96 + r) * 8 + (((3 - kq) ^ ((0 - (r >> 2)) & 3)) << 1));
            }
        }
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const double a1 = (MODE & 1) ? xf[s].x + xm[s].y : xf[s].x, a2 = (MODE & 1) ? xf[s].x - xm[s].y : xm[s].y;
            acc_a[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, be.x, acc_a[s], 0, 0, 0);
            acc_b[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bo.x, acc_b[s], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const double a1 = (MODE & 1) ? xf[s].y + xm[s].x : xf[s].y, a2 = (MODE & 1) ? xf[s].y - xm[s].x : xm[s].x;
            acc_a[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, be.y, acc_a[s], 0, 0, 0);
            acc_b[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bo.y, acc_b[s], 0, 0, 0);
        }
        if (!(MODE & 2)) { be.x += 1e-9; bo.y -= 1e-9; }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    double sum = 0;
    for (int s = 0; s < 6; ++s) sum += acc_a[s][0] + acc_b[s][1] + acc_a[s][2] + acc_b[s][3];
    if (sum == 12345.678) sink[0] = sum;
    if (tid == 0) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
}

template <int MODE> void run(int wpc, const double* gbuf, unsigned long long* d_st, double* d_sink) {
    const int tiles = 20000, nblk = 256 * wpc;
    const size_t lds = 3 * 320 * 8 * 8;
    CK(hipFuncSetAttribute((const void*)tile_loop<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(tile_loop<MODE>, dim3(nblk), dim3(256), lds, 0, tiles, d_st, d_sink, gbuf);
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(tile_loop<MODE>, dim3(nblk), dim3(256), lds, 0, tiles, d_st, d_sink, gbuf);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 3;
    std::vector<unsigned long long> st(2 * nblk);
    CK(hipMemcpy(st.data(), d_st, 16 * nblk, hipMemcpyDeviceToHost));
    std::vector<double> clk(nblk), cyc(nblk);
    for (int i = 0; i < nblk; ++i) { clk[i] = (double)st[2 * i] / st[2 * i + 1] * 100e6; cyc[i] = (double)st[2 * i]; }
    std::sort(clk.begin(), clk.end()); std::sort(cyc.begin(), cyc.end());
    const double nm = 24.0 * tiles;
    printf("{\"mode\": %d, \"v_add\": %d, \"lds_reads\": %d, \"barrier\": %d, \"lds_dma\": %d, \"b_direct\": %d, \"wg_per_cu\": %d, \"ms\": %.3f, \"clock_GHz\": %.3f, "
           "\"cycles_per_mfma_per_simd\": %.2f, \"TFLOPs\": %.2f}\n", MODE, MODE & 1, (MODE >> 1) & 1, (MODE >> 2) & 1, (MODE >> 3) & 1, (MODE >> 4) & 1, wpc, ms,
           clk[nblk / 2] / 1e9, cyc[nblk / 2] / nm / wpc, nm * 2048.0 * 4 * nblk / (ms * 1e-3) / 1e12);
}

// ---- the shipped K loop (emi_ring2_body, SW = 2, BK = 16, CT = 1, three stages), and De / Do straight from L2 ------------------
// One tile = 16 MFMAs (2 states x even / odd x 4 k-steps).  The DMA is inline assembly with a counted vmcnt (the builtin above makes
// the compiler drain vmcnt in front of every LDS read: r02_notes.md section 9, so modes 15 / 31 compared two drained loops); the
// loop is software-pipelined as shipped: fragment reads of tile kt+1 and the DMA of tile kt+3 in the gaps between the MFMAs of tile kt.
//   FORM 0: a stage holds forward x, mirrored x, De, Do: 6 DMA pieces and 12 ds_read_b128 per wave and tile
//   FORM 1: a stage holds x only (2 pieces, 8 reads); the wave's De / Do fragments of tile kt+1 come by four contiguous 1 KB
//           global_load_dwordx4 from a fragment-order copy (element (((ct*4 + w)*nkt + kt)*4 + q)*64 + lane), one tile ahead;
//           scalar base + constant 32-bit lane offset, the piece index as immediate offset
//   FORM 2: as 1, with a 64-bit per-lane address
// Operands: 64 instances x 6 states x 1024 nodes of x, De / Do of a 1024-node mesh; a workgroup sweeps the 32 K tiles of its
// column tile again and again; an XCD sees one column tile and four x tiles, so every operand is L2-resident.
typedef double d2 __attribute__((ext_vector_type(2)));
constexpr int PM = 1024, PH = PM / 2, PNKT = PH / 16, PNS = 6;

template <int FORM>
__global__ __launch_bounds__(256, 2) void kloop(int tiles, unsigned long long* stamps, double* sink, const double* X, const double* D, const d2* F) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int BK = 16, CH = 8, SW = 2, TM = 32, TN = 64, NST = 3, KH = 2;
    constexpr int ROWS = FORM ? 2 * TM : 2 * TM + 2 * TN;
    constexpr int STAGE = ROWS * BK, L = ROWS * CH / 256;
    constexpr int NM = 16;
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = blockIdx.x & 7, grp = (blockIdx.x >> 3) & 3, inst0 = grp * 16, i0 = ct * TN;
    auto swz = [](int r) { return (r >> 1) & 7; };
    unsigned voff[L]; unsigned long long gbase[L], gnext[L]; int gstep[L];
#pragma unroll
    for (int t = 0; t < L; ++t) {
        const int row0 = (wid + 4 * t) * 8, row = row0 + lane / CH, p = lane % CH;
        if (row0 < 2 * TM) {
            const bool mir = row0 >= TM;
            const int rr = row - (mir ? TM : 0), c = p ^ swz(rr);
            voff[t] = (unsigned)((((size_t)(inst0 + (rr & 15)) * PNS + (rr >> 4)) * PM + 2 * c) * 8);
            gbase[t] = (unsigned long long)(X + (mir ? PM - BK : 0));
            gstep[t] = mir ? -BK * 8 : BK * 8;
        } else {
            const bool od = row0 >= 2 * TM + TN;
            const int rr = row - 2 * TM - (od ? TN : 0), c = p ^ swz(rr);
            voff[t] = (unsigned)(((size_t)(i0 + rr) * PH + 2 * c) * 8);
            gbase[t] = (unsigned long long)(D + (od ? (size_t)PH * PH : 0));
            gstep[t] = BK * 8;
        }
        gnext[t] = gbase[t];
    }
    const unsigned lds0 = (unsigned)(unsigned long)(lds_ptr_t)smem;
    unsigned st_dma = 0, st_rd = 0;
    int nd = 0;                                         // K tile (of 32) the next DMA tile is
    auto issue_one = [&](int t) {
        const unsigned dst = lds0 + st_dma + (unsigned)(wid + 4 * t) * 1024u;
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff[t]), "s"(gnext[t]), "s"(dst) : "memory", "m0");
        gnext[t] = nd == PNKT - 1 ? gbase[t] : gnext[t] + (long long)gstep[t];
        if (t == L - 1) {
            st_dma = st_dma == (unsigned)((NST - 1) * STAGE * 8) ? 0u : st_dma + (unsigned)(STAGE * 8);
            nd = nd == PNKT - 1 ? 0 : nd + 1;
        }
    };
    // direct loads: the wave's 4 KB of tile kd in fragment order
    const unsigned long long fbase = (unsigned long long)(F + (size_t)(ct * 4 + wid) * PNKT * 256);
    unsigned long long fnext = fbase;                   // wave-uniform (FORM 1)
    const d2* flane = F + (size_t)(ct * 4 + wid) * PNKT * 256 + lane;   // per lane (FORM 2)
    const d2* fl = flane;
    const unsigned foff = (unsigned)lane * 16u;
    int kd = 0;
    struct Frag { d2 be[KH], bo[KH], sp[SW][KH], dm[SW][KH]; };
    auto dload_one = [&](Frag& f, int q) {              // q = 2h + odd
        d2& dst = (q & 1) ? f.bo[q >> 1] : f.be[q >> 1];
        if (FORM == 1) {
            if (q == 0) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(foff), "s"(fnext) : "memory");
            if (q == 1) asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(dst) : "v"(foff), "s"(fnext) : "memory");
            if (q == 2) asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048" : "=v"(dst) : "v"(foff), "s"(fnext) : "memory");
            if (q == 3) asm volatile("global_load_dwordx4 %0, %1, %2 offset:3072" : "=v"(dst) : "v"(foff), "s"(fnext) : "memory");
        } else {
            if (q == 0) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(fl) : "memory");
            if (q == 1) asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(dst) : "v"(fl) : "memory");
            if (q == 2) asm volatile("global_load_dwordx4 %0, %1, off offset:2048" : "=v"(dst) : "v"(fl) : "memory");
            if (q == 3) asm volatile("global_load_dwordx4 %0, %1, off offset:3072" : "=v"(dst) : "v"(fl) : "memory");
        }
        if (q == 3) {
            kd = kd == PNKT - 1 ? 0 : kd + 1;
            fnext = kd == 0 ? fbase : fnext + 4096;
            fl = kd == 0 ? flane : fl + 256;
        }
    };
    // the counted wait ahead of a tile's barrier: all but the youngest n loads have landed; the directly loaded fragments pass
    // through it as in / out operands, so no copy or use of them can be scheduled ahead of it
    auto wait_x = [&](Frag& f) {
        if (FORM == 0) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2)" : "+v"(f.be[0]), "+v"(f.bo[0]), "+v"(f.be[1]), "+v"(f.bo[1]) :: "memory");
    };
    int off_b[KH], off_f[SW][KH], off_m[SW][KH];
    const int rb = wid * 16 + r16;
#pragma unroll
    for (int h = 0; h < KH; ++h) off_b[h] = rb * BK + (((kq + 4 * h) ^ swz(rb)) << 1);
#pragma unroll
    for (int s = 0; s < SW; ++s)
#pragma unroll
        for (int h = 0; h < KH; ++h) {
            const int r = s * 16 + r16;
            off_f[s][h] = r * BK + (((kq + 4 * h) ^ swz(r)) << 1);
            off_m[s][h] = (TM + r) * BK + (((CH - 1 - kq - 4 * h) ^ swz(r)) << 1);
        }
    d2 txf[SW][KH], txm[SW][KH];
    constexpr int NRH = FORM ? 2 * SW : 2 + 2 * SW, NR = NRH * KH, NB = FORM ? 0 : 2;
    auto read_one = [&](Frag& f, const double* S, int r) {
        const int h = r / NRH, q = r % NRH;
        if (q < NB) {
            if (q & 1) f.bo[h] = *reinterpret_cast<const d2*>(S + (2 * TM + TN) * BK + off_b[h]);
            else f.be[h] = *reinterpret_cast<const d2*>(S + 2 * TM * BK + off_b[h]);
        } else if (q & 1) txm[(q - NB) >> 1][h] = *reinterpret_cast<const d2*>(S + off_m[(q - NB) >> 1][h]);
        else txf[(q - NB) >> 1][h] = *reinterpret_cast<const d2*>(S + off_f[(q - NB) >> 1][h]);
    };
    auto sums_one = [&](Frag& f, int s) {
#pragma unroll
        for (int h = 0; h < KH; ++h) {
            f.sp[s][h] = d2{txf[s][h].x + txm[s][h].y, txf[s][h].y + txm[s][h].x};
            f.dm[s][h] = d2{txf[s][h].x - txm[s][h].y, txf[s][h].y - txm[s][h].x};
        }
    };
    auto rd_stage = [&]() -> const double* {
        const double* S = smem + (st_rd >> 3);
        st_rd = st_rd == (unsigned)((NST - 1) * STAGE * 8) ? 0u : st_rd + (unsigned)(STAGE * 8);
        return S;
    };
    d4 acc_a[SW], acc_b[SW];
    for (int s = 0; s < SW; ++s) { acc_a[s] = d4{0, 0, 0, 0}; acc_b[s] = d4{0, 0, 0, 0}; }
    auto mfma_one = [&](const Frag& f, int i) {
        const int q = i % (2 * SW), j = i / (2 * SW), h = j >> 1, s = q >> 1;
        const bool second = j & 1;
        if (!(q & 1)) acc_a[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(second ? f.sp[s][h].y : f.sp[s][h].x, second ? f.be[h].y : f.be[h].x, acc_a[s], 0, 0, 0);
        else          acc_b[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(second ? f.dm[s][h].y : f.dm[s][h].x, second ? f.bo[h].y : f.bo[h].x, acc_b[s], 0, 0, 0);
    };
    // gaps of a tile's 16 MFMAs.  FORM 0 (as shipped): 2 reads in each of the first 6, a DMA piece in each of the next 6.
    // Direct: a direct load and 2 x reads in each of the first 4, a DMA piece in each of the next 2.
    constexpr int RPG = 2, GR = NR / RPG;
    auto step = [&](const Frag& cur, Frag& nxt) {
        wait_x(const_cast<Frag&>(cur));
        __builtin_amdgcn_s_waitcnt(0xC07F);
        asm volatile("s_barrier" ::: "memory");
        const double* S = rd_stage();
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            mfma_one(cur, i);
            if (FORM && i < 4) dload_one(nxt, i);
            if (i < GR) {
#pragma unroll
                for (int r = i * RPG; r < (i + 1) * RPG; ++r) read_one(nxt, S, r);
            } else if (i < GR + L) issue_one(i - GR);
            if (i >= NM - SW) sums_one(nxt, i - (NM - SW));
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    Frag f0, f1;
#pragma unroll
    for (int t = 0; t < L; ++t) issue_one(t);
#pragma unroll
    for (int t = 0; t < L; ++t) issue_one(t);
    if (FORM) {
#pragma unroll
        for (int q = 0; q < 4; ++q) dload_one(f0, q);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(f0.be[0]), "+v"(f0.bo[0]), "+v"(f0.be[1]), "+v"(f0.bo[1]) :: "memory");
    } else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
#pragma unroll
    for (int t = 0; t < L; ++t) issue_one(t);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    {
        const double* S = rd_stage();
#pragma unroll
        for (int r = 0; r < NR; ++r) read_one(f0, S, r);
#pragma unroll
        for (int s = 0; s < SW; ++s) sums_one(f0, s);
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int kt = 0; kt < tiles; kt += 2) {
        step(f0, f1);
        step(f1, f0);
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(f0.be[0]), "+v"(f0.bo[0]), "+v"(f0.be[1]), "+v"(f0.bo[1]) :: "memory");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    double sum = f0.be[0].x + f0.bo[1].y;
    for (int s = 0; s < SW; ++s) sum += acc_a[s][0] + acc_b[s][1] + acc_a[s][2] + acc_b[s][3];
    sink[(size_t)blockIdx.x * 256 + tid] = sum;          // (compared between the forms on the host: same operands, same order)
    if (tid == 0) { stamps[2 * blockIdx.x] = t1 - t0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
}

template <int FORM> void run_kloop(int wpc, const double* X, const double* D, const d2* F, unsigned long long* d_st, double* d_sink, std::vector<double>& out) {
    const int tiles = PNKT * 200, nblk = 256 * wpc;
    const size_t lds = (size_t)3 * (FORM ? 64 : 192) * 16 * 8;
    CK(hipFuncSetAttribute((const void*)kloop<FORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(kloop<FORM>, dim3(nblk), dim3(256), lds, 0, tiles, d_st, d_sink, X, D, F);
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(kloop<FORM>, dim3(nblk), dim3(256), lds, 0, tiles, d_st, d_sink, X, D, F);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 3;
    std::vector<unsigned long long> st(2 * nblk);
    CK(hipMemcpy(st.data(), d_st, 16 * nblk, hipMemcpyDeviceToHost));
    out.resize((size_t)nblk * 256);
    CK(hipMemcpy(out.data(), d_sink, out.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> clk(nblk), cyc(nblk);
    for (int i = 0; i < nblk; ++i) { clk[i] = (double)st[2 * i] / st[2 * i + 1] * 100e6; cyc[i] = (double)st[2 * i]; }
    std::sort(clk.begin(), clk.end()); std::sort(cyc.begin(), cyc.end());
    const double nm = 16.0 * tiles;
    printf("{\"probe\": \"kloop\", \"form\": \"%s\", \"dma_pieces\": %d, \"wg_per_cu\": %d, \"ms\": %.3f, \"clock_GHz\": %.3f, \"cycles_per_mfma_per_simd\": %.2f, "
           "\"cycles_per_tile_per_wave\": %.0f, \"TFLOPs\": %.2f}\n", FORM == 0 ? "all DMA" : FORM == 1 ? "De/Do direct, saddr" : "De/Do direct, 64-bit vaddr",
           FORM ? 2 : 6, wpc, ms, clk[nblk / 2] / 1e9, cyc[nblk / 2] / nm / wpc, cyc[nblk / 2] / tiles, nm * 2048.0 * 4 * nblk / (ms * 1e-3) / 1e12);
}

int main() {
    double *gbuf, *d_sink; unsigned long long* d_st;
    CK(hipMalloc(&gbuf, (size_t)8 << 20)); CK(hipMemset(gbuf, 0, (size_t)8 << 20));
    CK(hipMalloc(&d_sink, (size_t)512 * 256 * 8)); CK(hipMalloc(&d_st, 16 * 512));
    {
        // operands of the K-loop forms: x, row-major De | Do, and the same panels in fragment order
        std::vector<double> hx((size_t)64 * PNS * PM), hd((size_t)2 * PH * PH);
        std::vector<d2> hf((size_t)PH * PH);
        unsigned long long sd = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() { sd = sd * 6364136223846793005ull + 1442695040888963407ull; return (double)(long long)(sd >> 11) / 9007199254740992.0 - 0.5; };
        for (auto& v : hx) v = rnd();
        for (auto& v : hd) v = rnd();
        for (int c = 0; c < PH / 64; ++c)
            for (int w = 0; w < 4; ++w)
                for (int kt = 0; kt < PNKT; ++kt)
                    for (int q = 0; q < 4; ++q)
                        for (int l = 0; l < 64; ++l) {
                            const double* P = hd.data() + (q & 1 ? (size_t)PH * PH : 0) + (size_t)(64 * c + 16 * w + (l & 15)) * PH + 16 * kt + 8 * (q >> 1) + 2 * (l >> 4);
                            hf[((((size_t)c * 4 + w) * PNKT + kt) * 4 + q) * 64 + l] = d2{P[0], P[1]};
                        }
        double *dX, *dD; d2* dF;
        CK(hipMalloc(&dX, hx.size() * 8)); CK(hipMalloc(&dD, hd.size() * 8)); CK(hipMalloc(&dF, hf.size() * 16));
        CK(hipMemcpy(dX, hx.data(), hx.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(dD, hd.data(), hd.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(dF, hf.data(), hf.size() * 16, hipMemcpyHostToDevice));
        for (int wpc = 1; wpc <= 2; ++wpc) {
            std::vector<double> o0, o1, o2;
            run_kloop<0>(wpc, dX, dD, dF, d_st, d_sink, o0);
            run_kloop<1>(wpc, dX, dD, dF, d_st, d_sink, o1);
            run_kloop<2>(wpc, dX, dD, dF, d_st, d_sink, o2);
            size_t bad = 0;
            for (size_t i = 0; i < o0.size(); ++i) bad += (o0[i] != o1[i]) + (o0[i] != o2[i]);
            printf("{\"probe\": \"kloop\", \"wg_per_cu\": %d, \"sums_differing_from_all_dma\": %zu, \"of\": %zu}\n", wpc, bad, 2 * o0.size());
        }
        CK(hipFree(dX)); CK(hipFree(dD)); CK(hipFree(dF));
        if (getenv("MFMA_MIX_KLOOP_ONLY")) return 0;
    }
    for (int wpc = 1; wpc <= 2; ++wpc) {
        run<0>(wpc, gbuf, d_st, d_sink);
        run<1>(wpc, gbuf, d_st, d_sink);
        run<2>(wpc, gbuf, d_st, d_sink);
        run<3>(wpc, gbuf, d_st, d_sink);
        run<7>(wpc, gbuf, d_st, d_sink);
        run<15>(wpc, gbuf, d_st, d_sink);
        run<31>(wpc, gbuf, d_st, d_sink);
    }
    return 0;
}
