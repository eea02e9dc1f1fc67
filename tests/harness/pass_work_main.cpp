// pass_work_main.cpp -- the work table of the one-launch pass (etol_amd/csrc/emi_pass_work.hpp: pass_work_build over pass_role_of and
// ring_tile_of; its key from the plan, emi_pass_plan.hpp) as a stand-alone program under the host sanitizers (`make check-pass-work`):
// no Python, no device.  Over both built-in fp64 models, every SW their forms take, meshes, batches, block orders, tile orders (column
// partitions and the grouped order where plan_symdefect admits them), K slices and K halves it holds that
//   * the entry of every block of the grid is what pass_role_of and ring_tile_of return for it (worked out here, block by block,
//     as the kernel used to);
//   * every (tile, K slice) is visited exactly once, and so is every node chunk;
//   * every remaining block is idle;
//   * a launch that does not fit the fields of an entry is refused, not truncated.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "emi_pass_plan.hpp"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            if (++failures <= 20) {                              \
                std::fprintf(stderr, "FAILED %s: ", #cond);      \
                std::fprintf(stderr, __VA_ARGS__);               \
                std::fprintf(stderr, "\n");                      \
            }                                                    \
            return;                                              \
        }                                                        \
    } while (0)

struct Model { const char* name; int ns; std::vector<int> sw; };
const Model MODELS[] = {{"pointmass2", 2, {1, 2}}, {"quadrotor6", 6, {1, 2, 3, 6}}};
const int MESHES[] = {128, 256, 1024};
const int BATCHES[] = {1, 3, 16, 17, 80, 128, 160, 320, 704, 1024, 2048, 4096};
const int ORDERS[] = {0, 1, 110, 150, 400};
const int CPARTS[] = {0, 1, 2, 4, 8};
const int GBLKS[] = {1, 2, 4};      // the grouped order: SymPlan::cpart -1, -2, -4
const int KSPLITS[] = {1, 2, 4};

long long cases = 0, grouped = 0, partitioned = 0, idle_blocks = 0;

void one_case(const Model& m, int sw, int M, int B, int order, int cpart_opt, int gblk, int ksplit, int hs, int ctc) {
    emi::SymPlan p = emi::plan_symdefect(m.ns, B, M, emi::symdefect_ct_of(m.ns, sw), emi::legal_ks((M / 2) / 8, ksplit), cpart_opt, gblk, 0, 8, ctc);
    if (p.ring1 || p.sw != sw || p.ct != ctc) return;       // (no such launch)
    if (gblk > 0 && p.cpart >= 0) return;                    // (plan_symdefect does not admit the grouped order here)
    if (cpart_opt > 0 && p.cpart != cpart_opt && !(cpart_opt == 1 && p.cpart == 0)) return;      // (... nor these column partitions)
    p.hs = hs;
    const emi::PassWorkKey k = emi::pass_work_for(p, m.ns, B, M, order);
    std::vector<emi::PassWork> table;
    const char* why = "";
    CHECK(emi::pass_work_build(k, table, &why), "%s sw %d M %d B %d: build refused (%s)", m.name, sw, M, B, why);
    ++cases;
    grouped += p.cpart < 0;
    partitioned += p.cpart > 0;
    // the counts are the launcher's
    const int mtiles = (B + 15) / 16, ntiles = (M / 2) / (64 * ctc), nsg = m.ns / sw;
    CHECK(k.nm == mtiles * ntiles * nsg * p.ks && k.nn == ((M + 511) / 512) * B && k.nm8 == (k.nm + 7) / 8 && k.nn8 == ((k.nn + hs - 1) / hs + 7) / 8,
          "%s sw %d M %d B %d ks %d hs %d: counts", m.name, sw, M, B, p.ks, hs);
    CHECK((long long)table.size() == 8LL * (k.nm8 + k.nn8), "table size");
    std::vector<unsigned char> tile_seen((size_t)k.nm, 0), chunk_seen((size_t)k.nn, 0);
    for (int g = 0; g < (int)table.size(); ++g) {
        const emi::PassWork e = table[(size_t)emi::pass_work_index(g, k.per_xcd())];
        // what the kernel worked out for block g before it read a table
        const int xcd = g & 7, j = g >> 3;
        const emi::PassRole role = emi::pass_role_of(j, k.nm8, k.nn8, order);
        if (role.mfma) {
            const int tid = xcd * k.nm8 + role.index;
            if (tid >= k.nm) {
                CHECK(e.w0 == 0 && e.w1 == 0, "block %d: not idle", g);
                ++idle_blocks;
                continue;
            }
            const emi::RingTile rt = emi::ring_tile_of(tid / p.ks, ntiles, mtiles * nsg, p.cpart, p.cx, nsg);
            CHECK(emi::pass_work_role(e) == emi::PASS_WORK_MFMA && emi::pass_work_ntile(e) == rt.ntile && emi::pass_work_grp(e) == rt.grp &&
                      emi::pass_work_kslice(e) == tid % p.ks,
                  "%s sw %d M %d B %d order %d cpart %d cx %d ks %d: block %d holds (%d, %d, %d), the maps say (%d, %d, %d)", m.name, sw, M, B, order,
                  p.cpart, p.cx, p.ks, g, emi::pass_work_ntile(e), emi::pass_work_grp(e), emi::pass_work_kslice(e), rt.ntile, rt.grp, tid % p.ks);
            const size_t at = ((size_t)rt.grp * ntiles + rt.ntile) * p.ks + tid % p.ks;
            CHECK(at < tile_seen.size() && !tile_seen[at], "(tile, slice) %zu visited twice or out of range", at);
            tile_seen[at] = 1;
        } else {
            bool any = false;
            for (int half = 0; half < hs; ++half) {
                const int nid = (xcd * k.nn8 + role.index) * hs + half;
                if (nid >= k.nn) {
                    CHECK(half == 0 ? (e.w0 == 0 && e.w1 == 0) : !emi::pass_work_has_chunk(e, 1), "block %d half %d: not idle", g, half);
                    continue;
                }
                any = true;
                CHECK(emi::pass_work_role(e) == emi::PASS_WORK_NODE && emi::pass_work_has_chunk(e, half) && emi::pass_work_bx(e, half) == nid % k.nbx &&
                          emi::pass_work_b(e, half) == nid / k.nbx,
                      "%s M %d B %d order %d hs %d: block %d half %d holds (%d, %d), the kernel's formula says (%d, %d)", m.name, M, B, order, hs, g,
                      half, emi::pass_work_bx(e, half), emi::pass_work_b(e, half), nid % k.nbx, nid / k.nbx);
                CHECK(!chunk_seen[(size_t)nid], "node chunk %d visited twice", nid);
                chunk_seen[(size_t)nid] = 1;
            }
            idle_blocks += !any;
        }
    }
    for (size_t i = 0; i < tile_seen.size(); ++i) CHECK(tile_seen[i], "%s sw %d M %d B %d: (tile, slice) %zu never visited", m.name, sw, M, B, i);
    for (size_t i = 0; i < chunk_seen.size(); ++i) CHECK(chunk_seen[i], "%s M %d B %d hs %d: node chunk %zu never visited", m.name, M, B, hs, i);
}

void refusals() {
    std::vector<emi::PassWork> t;
    const char* why = "";
    emi::PassWorkKey k = emi::pass_work_key(6, 64, 1024, 2, 1, 1, 1, 0, 0, 0);
    CHECK(emi::pass_work_build(k, t, &why), "plain key refused (%s)", why);
    emi::PassWorkKey bad = k;
    bad.ks = 512;
    bad.nm = k.nm * 512;
    bad.nm8 = (bad.nm + 7) / 8;
    CHECK(!emi::pass_work_build(bad, t, &why), "512 K slices fit no entry");
    bad = k;
    bad.nbx = 1 << 15;
    bad.nn = bad.nbx * 64;
    bad.nn8 = (bad.nn + 7) / 8;
    CHECK(!emi::pass_work_build(bad, t, &why), "32768 node chunks per instance fit no entry");
    bad = k;
    bad.nm8 -= 1;       // fewer workgroups than tiles
    CHECK(!emi::pass_work_build(bad, t, &why), "a grid short of its tiles");
    bad = k;
    bad.ngrp += 1;      // tiles that do not add up to the count
    CHECK(!emi::pass_work_build(bad, t, &why), "tiles that do not add up");
    // the widest fields that fit: 256 K slices
    emi::PassWorkKey wide = k;
    wide.ks = 256;
    wide.nm = k.nm * 256;
    wide.nm8 = (wide.nm + 7) / 8;
    CHECK(emi::pass_work_build(wide, t, &why), "256 K slices refused (%s)", why);
    CHECK(emi::pass_work_kslice(t[(size_t)emi::pass_work_index(8 * (wide.nm8 - 1), wide.per_xcd())]) <= 255, "K slice field");
}

}  // namespace

int main() {
    for (const Model& m : MODELS)
        for (int sw : m.sw)
            for (int M : MESHES)
                for (int B : BATCHES)
                    for (int order : ORDERS)
                        for (int ksplit : KSPLITS)
                            for (int hs = 1; hs <= 2; ++hs) {
                                for (int cp : CPARTS) one_case(m, sw, M, B, order, cp, 0, ksplit, hs, 1);
                                for (int g : GBLKS) one_case(m, sw, M, B, order, 0, g, ksplit, hs, 1);
                                if (sw == 2 && m.ns > 2 && M % 256 == 0 && ksplit == 1) one_case(m, sw, M, B, order, 0, B % 256 == 0 ? 2 : 0, 1, hs, 2);
                            }
    refusals();
    std::printf("pass work: %lld tables, %lld in the grouped order, %lld in column partitions, %lld idle blocks, %d failures\n", cases, grouped, partitioned,
                idle_blocks, failures);
    if (failures || cases < 10000 || grouped < 100 || partitioned < 1000) return 1;
    std::printf("pass work: ok\n");
    return 0;
}
