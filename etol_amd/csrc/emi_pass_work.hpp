// emi_pass_work.hpp -- which workgroup of the one-launch pass does what: the two maps that define the order (ring_tile_of,
// pass_role_of), and the WORK TABLE the host builds from them, one 8-byte entry per block of the launch grid, which
// emi_pass_f64_kernel reads instead of working the maps out again in every workgroup (two 64-bit and up to twelve 32-bit integer
// divisions ahead of the first memory request of each of them).  Batch, mesh and plan stay the same from call to call of an NLP
// iteration or a lock-step solve, and so do the answers: a context keeps the tables of its last launches (emi_api_pass.hip).
// The first part is shared with the kernels and with model programs compiled at run time, so it includes nothing; the builder
// below it is host-only and compiles with a plain C++ compiler (tests/harness/pass_work_main.cpp, `make check-pass-work`).
#pragma once

#if defined(__HIPCC__)
#define EMI_WORK_HD __host__ __device__
#else
#define EMI_WORK_HD
#endif

namespace emi {

// Which tile a workgroup of the state-split ring kernel works on.  tl counts tiles in XCD-local runs (an XCD gets a contiguous
// range of the launch); ntiles column tiles, ngrp (instance group x state group) rows of tiles.  cpart = 0: plain order, the
// column tiles of a group are neighbours.  cpart > 0: XCD x works on column partition x % cpart (ntiles / cpart columns, cx of
// them interleaved at a time: cx divides that count) and on group partition x / cpart (ngrp cpart / 8 groups).  cpart < 0: the
// grouped order described in the function (G = -cpart instance groups per super-block, nsg state groups per instance group;
// needs (ngrp / nsg) % (8 G) == 0 and ntiles % cx == 0: plan_symdefect checks).  One function for
// the kernel and for the host-side check that every tile is visited exactly once (emi_debug_tile_order, tests/test_abi.py).
struct RingTile { int ntile, grp; };
EMI_WORK_HD inline RingTile ring_tile_of(int tl, int ntiles, int ngrp, int cpart, int cx, int nsg = 1) {
    RingTile t;
    if (cpart > 0) {
        const int per_xcd = ngrp * ntiles / 8;
        const int x = tl / per_xcd, m = tl - x * per_xcd;
        const int pc = x % cpart, pg = x / cpart;
        const int ncol = ntiles / cpart, ng = ngrp / (8 / cpart);
        const int cb = m / (ng * cx), r = m - cb * ng * cx;
        t.grp = pg * ng + r / cx;
        t.ntile = pc * ncol + cb * cx + r % cx;
    } else if (cpart < 0) {
        // Grouped order (cpart = -G): an XCD keeps its own contiguous range of instance groups (the range whose node-role
        // workgroups it also runs in the one-launch pass) and walks it in super-blocks of G groups; inside a super-block the
        // column tiles go in blocks of cx, and for one column block all G groups x nsg state groups run before the next
        // block.  X and U of a super-block are then fetched into this XCD's L2 once, by whichever role gets there first,
        // and a column block's share of De / Do is walked once per super-block instead of once per (group, state group).
        const int G = -cpart, per_xcd = ngrp * ntiles / 8;
        const int x = tl / per_xcd, m = tl - x * per_xcd;
        const int per_sb = G * nsg * ntiles, sb = m / per_sb, r = m - sb * per_sb;
        const int per_cb = G * nsg * cx, cb = r / per_cb, r2 = r - cb * per_cb;
        const int g = r2 / (nsg * cx), r3 = r2 - g * (nsg * cx);
        const int mt = x * (ngrp / nsg / 8) + sb * G + g;
        t.grp = mt * nsg + r3 / cx;
        t.ntile = cb * cx + r3 % cx;
    } else {
        t.ntile = tl % ntiles;
        t.grp = tl / ntiles;
    }
    return t;
}
// Role of block j of an XCD's share of the one-launch pass grid (nm MFMA-role and nn node-role blocks): {is_mfma, index within
// the role}.  order 0: evenly interleaved; 1: all MFMA blocks first; >= 100: interleaved with the MFMA blocks at order / 100 times
// the even density until they are used up, node blocks at the tail (a density beyond one MFMA block per block saturates HERE at
// order 1, which keeps the map a bijection for every caller: the first form of this map, unclamped, sent node workgroups out of range).  One function for the kernel and for the host-side check (emi_debug_pass_roles).
struct PassRole { int mfma, index; };
EMI_WORK_HD inline PassRole pass_role_of(int j, int nm, int nn, int order) {
    const long long t = (long long)nm + nn;
    long long m0, m1;
    const long long d = order >= 100 ? order : 100;
    // a density beyond one MFMA block per block (d nm > 100 t) would deal two MFMA indices to one block -- the map would no
    // longer be a bijection: it saturates HERE, for every caller, at "all MFMA blocks first"
    if (order == 1 || d * nm > 100 * t) {
        m0 = j < nm ? j : nm;
        m1 = j < nm ? j + 1 : nm;
    } else {
        m0 = ((long long)j * nm * d) / (100 * t);
        m1 = ((long long)(j + 1) * nm * d) / (100 * t);
        if (m0 > nm) m0 = nm;
        if (m1 > nm) m1 = nm;
    }
    PassRole r;
    r.mfma = m1 > m0;
    r.index = (int)(r.mfma ? m0 : j - m0);
    return r;
}

// ---- the work table: what block g of the grid of emi_pass_f64_kernel does -------------------------------------------------------
// One entry of two words per block.  Block g belongs to XCD g % 8 and is its block j = g / 8; the entries of an XCD are
// neighbours ([xcd][j], per_xcd = MFMA + node workgroups per XCD), so its consecutive blocks share 64-byte lines.
//   w0 bits 0-1: the role (idle: the block returns at once; the whole entry is zero);
//   MFMA role:  w0 bits 2-9 the K slice, bits 10-31 the column tile; w1 the group (instance group x state group);
//   node role:  w0 bits 4-17 the chunk bx of the workgroup's first 256 threads, w1 its instance b; a workgroup of 512 threads
//               (K halves, HS = 2) takes the next chunk too: bit 2 says that there is one, bits 18-31 hold its bx, bit 3 that it
//               belongs to instance b + 1.
struct PassWork { unsigned w0, w1; };
enum PassWorkRole { PASS_WORK_IDLE = 0, PASS_WORK_MFMA = 1, PASS_WORK_NODE = 2 };
constexpr unsigned PASS_WORK_MAX_KSLICE = 1u << 8, PASS_WORK_MAX_NTILE = 1u << 22, PASS_WORK_MAX_BX = 1u << 14;

EMI_WORK_HD inline long long pass_work_index(int g, int per_xcd) { return (long long)(g & 7) * per_xcd + (g >> 3); }
EMI_WORK_HD inline int pass_work_role(PassWork e) { return (int)(e.w0 & 3u); }
EMI_WORK_HD inline int pass_work_kslice(PassWork e) { return (int)((e.w0 >> 2) & 255u); }
EMI_WORK_HD inline int pass_work_ntile(PassWork e) { return (int)(e.w0 >> 10); }
EMI_WORK_HD inline int pass_work_grp(PassWork e) { return (int)e.w1; }
// node role, half 0 / 1 of the workgroup (HS = 1: half 0 only)
EMI_WORK_HD inline bool pass_work_has_chunk(PassWork e, int half) { return half == 0 || (e.w0 & 4u) != 0; }
EMI_WORK_HD inline int pass_work_bx(PassWork e, int half) { return (int)((e.w0 >> (half ? 18 : 4)) & 0x3FFFu); }
EMI_WORK_HD inline int pass_work_b(PassWork e, int half) { return (int)e.w1 + (half ? (int)((e.w0 >> 3) & 1u) : 0); }

}  // namespace emi

#ifndef __HIPCC_RTC__
#include <vector>

namespace emi {

// Everything the entries depend on, and nothing else: the key of a context's cache of tables.
struct PassWorkKey {
    int nm = 0, nn = 0;         // MFMA workgroups (tiles x K slices) and node chunks of the launch
    int nm8 = 0, nn8 = 0;       // workgroups of either role per XCD (rounded up; a node workgroup takes hs chunks)
    int order = 0;              // block order (pass_role_of)
    int ntiles = 0, ngrp = 0;   // column tiles, (instance group x state group) rows of tiles
    int nsg = 1;                // state groups per instance group
    int cpart = 0, cx = 0;      // tile order (ring_tile_of)
    int ks = 1, hs = 1;         // K slices per tile, K halves (= node chunks) per workgroup
    int nbx = 1;                // node chunks per instance
    bool operator==(const PassWorkKey& o) const {
        return nm == o.nm && nn == o.nn && nm8 == o.nm8 && nn8 == o.nn8 && order == o.order && ntiles == o.ntiles && ngrp == o.ngrp && nsg == o.nsg &&
               cpart == o.cpart && cx == o.cx && ks == o.ks && hs == o.hs && nbx == o.nbx;
    }
    int per_xcd() const { return nm8 + nn8; }
    long long blocks() const { return 8LL * per_xcd(); }
};

// The key of a launch: B instances of ns states on M nodes, sw states and ct 64-column sub-tiles per MFMA workgroup, ks K slices per
// tile, hs K halves, the tile order (cpart, cx) and the block order.  The counts are those emi_pass_f64_kernel's launcher states.
inline PassWorkKey pass_work_key(int ns, int B, int M, int sw, int ct, int ks, int hs, int cpart, int cx, int order) {
    PassWorkKey k;
    const int mtiles = (B + 15) / 16;
    k.ks = ks > 1 ? ks : 1;
    k.hs = hs == 2 ? 2 : 1;
    k.nsg = ns / sw;
    k.ntiles = (M / 2) / (64 * ct);
    k.ngrp = mtiles * k.nsg;
    k.nm = k.ngrp * k.ntiles * k.ks;
    k.nbx = (M + 511) / 512;
    k.nn = k.nbx * B;
    k.nm8 = (k.nm + 7) / 8;
    k.nn8 = ((k.nn + k.hs - 1) / k.hs + 7) / 8;
    k.order = order;
    k.cpart = cpart;
    k.cx = cx;
    return k;
}

// The table of a key, [xcd][j], by calling pass_role_of and ring_tile_of themselves: they stay the only definition of the order.
// Blocks past the real counts (the rounding of nm8 / nn8) are idle.  false: the launch does not fit the fields of an entry or an
// index leaves its range (nothing is truncated; *why names the field).
inline bool pass_work_build(const PassWorkKey& k, std::vector<PassWork>& out, const char** why = nullptr) {
    const char* dummy;
    const char*& w = why ? *why : dummy;
    w = "";
    if (k.nm < 0 || k.nn < 1 || k.nm8 < 0 || k.nn8 < 1 || k.ntiles < 1 || k.ngrp < 1 || k.nsg < 1 || k.nbx < 1 || k.ks < 1 || k.hs < 1 || k.hs > 2) {
        w = "counts";
        return false;
    }
    if ((long long)k.nm8 * 8 < k.nm || (long long)k.nn8 * 8 * k.hs < k.nn) { w = "workgroups per XCD"; return false; }
    if (k.blocks() > 0x7FFFFFFFLL) { w = "grid"; return false; }
    if ((unsigned)k.ks > PASS_WORK_MAX_KSLICE) { w = "K slices"; return false; }
    if ((unsigned)k.ntiles > PASS_WORK_MAX_NTILE) { w = "column tiles"; return false; }
    if ((unsigned)k.nbx > PASS_WORK_MAX_BX) { w = "node chunks per instance"; return false; }
    if ((long long)k.ngrp * k.ntiles * k.ks != k.nm) { w = "tiles"; return false; }
    out.assign((size_t)k.blocks(), PassWork{0u, 0u});
    const int per = k.per_xcd();
    for (int xcd = 0; xcd < 8; ++xcd)
        for (int j = 0; j < per; ++j) {
            PassWork& e = out[(size_t)xcd * per + j];
            const PassRole role = pass_role_of(j, k.nm8, k.nn8, k.order);
            if (role.index < 0 || role.index >= (role.mfma ? k.nm8 : k.nn8)) { w = "role index"; return false; }
            if (role.mfma) {
                const long long bid = (long long)xcd * k.nm8 + role.index;      // tile-and-slice id, XCD-local runs
                if (bid >= k.nm) continue;
                const RingTile rt = ring_tile_of((int)(bid / k.ks), k.ntiles, k.ngrp, k.cpart, k.cx, k.nsg);
                if (rt.ntile < 0 || rt.ntile >= k.ntiles || rt.grp < 0 || rt.grp >= k.ngrp) { w = "tile"; return false; }
                e.w0 = (unsigned)PASS_WORK_MFMA | (unsigned)(bid % k.ks) << 2 | (unsigned)rt.ntile << 10;
                e.w1 = (unsigned)rt.grp;
            } else {
                const long long n0 = ((long long)xcd * k.nn8 + role.index) * k.hs;     // first node chunk of the workgroup
                if (n0 >= k.nn) continue;
                e.w0 = (unsigned)PASS_WORK_NODE | (unsigned)(n0 % k.nbx) << 4;
                e.w1 = (unsigned)(n0 / k.nbx);
                if (k.hs == 2 && n0 + 1 < k.nn)
                    e.w0 |= 4u | ((n0 + 1) / k.nbx != n0 / k.nbx ? 8u : 0u) | (unsigned)((n0 + 1) % k.nbx) << 18;
            }
        }
    return true;
}

}  // namespace emi
#endif
