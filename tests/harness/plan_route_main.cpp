// plan_route_main.cpp -- stand-alone check of the planned route (emi_plan_route: etol_amd/csrc/emi_host.cpp with emi_plan_route.hpp, host
// only), built with the host sanitizers (`make check-plan-route`).  It reads the fixtures of tests/golden/plan_cases.json (path in
// argv[1]) with the few lines of JSON reader below, runs every case on grids of 9, 17, 33 and 161 points and meshes of 3, 5, 33 and
// 130 LGL nodes, holds what can be held without a second implementation (the recorded level, a route of 8-adjacent cells from the
// start cell to the goal cell, end points kept, nothing written without a route, the refusals) and prints one JSON line per case
// and grid with the level, the cost and the route at 33 nodes as hexadecimal doubles, which tests/test_plan_route_cpu.py compares
// with the library's own answers bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "emi355x.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

// ---- JSON, as much of it as the fixture uses: objects, arrays, strings without escapes, numbers, null
struct Value {
    enum Kind { NUL, NUM, STR, ARR, OBJ } kind = NUL;
    double num = 0;
    std::string str;
    std::vector<Value> arr;
    std::map<std::string, Value> obj;
    const Value& at(const std::string& k) const { return obj.at(k); }
};

struct Reader {
    const std::string& s;
    size_t p = 0;
    explicit Reader(const std::string& text) : s(text) {}
    void skip() { while (p < s.size() && (s[p] == ' ' || s[p] == '\n' || s[p] == '\t' || s[p] == '\r' || s[p] == ',' || s[p] == ':')) ++p; }
    [[noreturn]] void fail(const char* what) { std::fprintf(stderr, "fixture: %s at byte %zu\n", what, p); std::exit(2); }
    std::string string() {
        const size_t e = s.find('"', p + 1);
        if (e == std::string::npos) fail("open string");
        const std::string out = s.substr(p + 1, e - p - 1);
        p = e + 1;
        return out;
    }
    Value value() {
        skip();
        Value v;
        if (p >= s.size()) fail("end of text");
        if (s[p] == '[') {
            v.kind = Value::ARR;
            for (++p;;) { skip(); if (p >= s.size()) fail("open array"); if (s[p] == ']') { ++p; break; } v.arr.push_back(value()); }
        } else if (s[p] == '{') {
            v.kind = Value::OBJ;
            for (++p;;) {
                skip();
                if (p >= s.size()) fail("open object");
                if (s[p] == '}') { ++p; break; }
                if (s[p] != '"') fail("key expected");
                const std::string k = string();
                v.obj[k] = value();
            }
        } else if (s[p] == '"') {
            v.kind = Value::STR;
            v.str = string();
        } else if (s.compare(p, 4, "null") == 0) {
            p += 4;
        } else {
            char* end = nullptr;
            v.kind = Value::NUM;
            v.num = std::strtod(s.c_str() + p, &end);
            if (end == s.c_str() + p) fail("number expected");
            p = (size_t)(end - s.c_str());
        }
        return v;
    }
};

std::vector<double> numbers(const Value& v) {
    std::vector<double> out;
    for (const Value& e : v.arr) {
        if (e.kind == Value::ARR) { for (const Value& q : e.arr) out.push_back(q.num); }
        else out.push_back(e.num);
    }
    return out;
}

void print_hex(const char* key, const std::vector<double>& v) {
    std::printf(", \"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s\"%a\"", i ? ", " : "", v[i]);
    std::printf("]");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s plan_cases.json\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::stringstream buf;
    buf << in.rdbuf();
    const std::string text = buf.str();
    const Value cases = Reader(text).value();
    EXPECT(cases.kind == Value::ARR && !cases.arr.empty());
    const double NaN = std::numeric_limits<double>::quiet_NaN();
    const int grids[] = {9, 17, 33, 161}, meshes[] = {3, 5, 33, 130};

    for (const Value& c : cases.arr) {
        const std::string name = c.at("name").str;
        const std::vector<double> recs = numbers(c.at("recs")), ends = numbers(c.at("ends"));
        const bool has_box = c.at("box").kind == Value::ARR;
        const std::vector<double> box = has_box ? numbers(c.at("box")) : std::vector<double>();
        const double clearance = c.at("clearance").num;
        const int np = (int)(recs.size() / EMI_PATH_REC);
        EXPECT(recs.size() % EMI_PATH_REC == 0 && ends.size() == 4 && (!has_box || box.size() == 4));
        for (int grid : grids) {
            const int want = (int)c.at("levels").at(std::to_string(grid)).num;
            std::vector<double> xs33, ys33;
            std::vector<int> cells33;
            double cost33 = 0;
            for (int M : meshes) {
                std::vector<double> tau(M), w(M), D((size_t)M * M), xs(M, NaN), ys(M, NaN);
                EXPECT(emi_lgl(M, tau.data(), w.data(), D.data()) == EMI_OK);
                std::vector<int> cells((size_t)grid * grid, -7);
                int level = 99, ncells = -1;
                double cost = NaN;
                EXPECT(emi_plan_route(np, recs.data(), ends.data(), has_box ? box.data() : nullptr, clearance, grid, M, tau.data(), xs.data(),
                                      ys.data(), &level, &cost, cells.data(), &ncells) == EMI_OK);
                EXPECT(level == want);
                if (level < 0) {
                    EXPECT(cost == 0.0 && ncells == 0 && std::isnan(xs[0]) && std::isnan(ys[M - 1]) && cells[0] == -7);
                } else {
                    EXPECT(ncells >= 2 && ncells <= grid * grid && cost > 0.0);
                    for (int n = 1; n < ncells; ++n) {
                        const int di = cells[n] / grid - cells[n - 1] / grid, dj = cells[n] % grid - cells[n - 1] % grid;
                        EXPECT(cells[n] >= 0 && cells[n] < grid * grid && std::abs(di) <= 1 && std::abs(dj) <= 1 && (di || dj));
                    }
                    EXPECT(cells[ncells] == -7);
                    EXPECT(xs[0] == ends[0] && ys[0] == ends[1] && xs[M - 1] == ends[2] && ys[M - 1] == ends[3]);
                    for (int k = 0; k < M; ++k) EXPECT(std::isfinite(xs[k]) && std::isfinite(ys[k]));
                }
                // without the optional outputs: the same route
                std::vector<double> xs2(M, NaN), ys2(M, NaN);
                int level2 = 99;
                EXPECT(emi_plan_route(np, recs.data(), ends.data(), has_box ? box.data() : nullptr, clearance, grid, M, tau.data(), xs2.data(),
                                      ys2.data(), &level2, nullptr, nullptr, nullptr) == EMI_OK);
                EXPECT(level2 == level);
                for (int k = 0; k < M && level >= 0; ++k) EXPECT(xs2[k] == xs[k] && ys2[k] == ys[k]);
                if (M == 33) { xs33 = xs; ys33 = ys; cost33 = cost; cells33.assign(cells.begin(), cells.begin() + ncells); }
                if (M == 33) {
                    std::printf("{\"case\": \"%s\", \"grid\": %d, \"level\": %d, \"cost\": \"%a\", \"cells\": [", name.c_str(), grid, level, cost33);
                    for (size_t n = 0; n < cells33.size(); ++n) std::printf("%s%d", n ? ", " : "", cells33[n]);
                    std::printf("]");
                    if (level < 0) { xs33.clear(); ys33.clear(); }
                    print_hex("xs", xs33);
                    print_hex("ys", ys33);
                    std::printf("}\n");
                }
            }
        }
    }

    // the refusals
    {
        const double rec[EMI_PATH_REC] = {1, 5, 0, 1, 0, 0, 0, 0}, ends[4] = {0, 0, 10, 0}, tau[3] = {-1, 0, 1};
        double xs[3], ys[3];
        int level = 0;
        const auto call = [&](int np, const double* r, const double* e, double cl, int grid, int M, const double* t, double* x, double* y, int* l) {
            return emi_plan_route(np, r, e, nullptr, cl, grid, M, t, x, y, l, nullptr, nullptr, nullptr);
        };
        EXPECT(call(1, rec, ends, 0.01, 0, 3, tau, xs, ys, &level) == EMI_OK && level == 0);
        EXPECT(call(-1, rec, ends, 0.01, 0, 3, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, nullptr, ends, 0.01, 0, 3, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, nullptr, 0.01, 0, 3, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, NaN, 0, 3, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, 8, 3, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, 162, 3, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, -1, 3, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, 0, 1, tau, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, 0, 3, nullptr, xs, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, 0, 3, tau, nullptr, ys, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, 0, 3, tau, xs, nullptr, &level) == EMI_ERR_ARG);
        EXPECT(call(1, rec, ends, 0.01, 0, 3, tau, xs, ys, nullptr) == EMI_ERR_ARG);
        EXPECT(call(0, nullptr, ends, 0.01, 9, 3, tau, xs, ys, &level) == EMI_OK && level == -2);      // no records: nothing to plan
        const double same[4] = {1, 1, 1, 1};
        EXPECT(call(1, rec, same, 0.01, 9, 3, tau, xs, ys, &level) == EMI_OK && level == -2);          // no span
        const double inf_ends[4] = {0, 0, HUGE_VAL, 0};
        EXPECT(call(1, rec, inf_ends, 0.01, 9, 3, tau, xs, ys, &level) == EMI_OK && level < 0);        // (no cell index is made of it)
    }
    if (failures) { std::fprintf(stderr, "plan route: %d failures\n", failures); return 1; }
    std::printf("plan route: ok\n");
    return 0;
}
