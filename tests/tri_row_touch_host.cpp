// Host check of csrc/tri_row_touch.h (compiled and run by test_tri_row_touch_host.py): for a row of L positions and a position stride zl,
//   - every offset the touch and the walk produce (inactive touch loads and clamped walk lanes included) lies inside the row's extent;
//   - the active touch loads of the three k-groups produce every 128-byte line of every position exactly once;
//   - the lines of k-group g are exactly the lines the walk of k-group g reads, and the walk reads every float of them exactly once.
// usage: tri_row_touch_host L zl      (prints one line, exit status 0 = all checks hold)
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "tri_row_touch.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int L = atoi(argv[1]);
    const long long zl = atoll(argv[2]);
    if (L < 1 || L > RFT_LMAX || zl < RFT_CH || zl % 4) return 2;
    const long long extent = (long long)(L - 1) * zl + RFT_CH;            // floats from z[b, s, 0, 0] to the end of the last position
    int bad = 0;
    auto fail = [&](const char* what, long long a, long long b, long long c) {
        if (bad++ < 10) fprintf(stderr, "L=%d zl=%lld: %s (%lld, %lld, %lld)\n", L, zl, what, a, b, c);
    };
    std::map<long long, int> touched;                                     // line start (floats) -> times produced over the k-groups
    std::vector<std::set<long long>> tlines(RFT_KGROUPS), wlines(RFT_KGROUPS);
    for (int g = 0; g < RFT_KGROUPS; ++g)
        for (int lane = 0; lane < RFT_LANES; ++lane)
            for (int i = 0; i < RFT_N; ++i) {
                const long long off = rf_touch_offset(L, zl, g, lane, i);
                if (off < 0 || off + 1 > extent) fail("touch offset outside the row", g, lane, i);
                if (!rf_touch_active(L, lane, i)) continue;
                if ((off % zl) % RFT_LINE) fail("touch offset not at a line start", g, lane, i);
                ++touched[off];
                tlines[g].insert(off);
            }
    // every line of every position exactly once
    for (int l = 0; l < L; ++l)
        for (int j = 0; j < RFT_CH / RFT_LINE; ++j) {
            const long long off = (long long)l * zl + j * RFT_LINE;
            auto it = touched.find(off);
            if (it == touched.end() || it->second != 1) fail("line not produced exactly once", l, j, it == touched.end() ? 0 : it->second);
        }
    if ((long long)touched.size() != (long long)L * (RFT_CH / RFT_LINE)) fail("lines beyond the row's positions", (long long)touched.size(), L, 0);
    // the walk: 11 computing waves x (32 positions x 2 channel halves), k-tiles 4 g .. 4 g + 3
    std::map<long long, int> floats;                                      // float offset -> times read by lanes whose position is inside the row
    const int waves = (RFT_LMAX + 31) / 32;
    for (int g = 0; g < RFT_KGROUPS; ++g)
        for (int w = 0; w < waves; ++w)
            for (int pr = 0; pr < 32; ++pr)
                for (int hh = 0; hh < 2; ++hh)
                    for (int kt = 4 * g; kt < 4 * g + 4; ++kt) {
                        const long long off = rf_walk_base(L, zl, w, pr, hh) + rf_walk_ktile(kt);
                        if (off < 0 || off + RFT_WALK_FLOATS > extent) fail("walk read outside the row", w, pr, kt);
                        if (32 * w + pr >= L) continue;                   // (a clamped lane reads the last position again)
                        for (int e = 0; e < RFT_WALK_FLOATS; ++e) {
                            ++floats[off + e];
                            const long long in_pos = (off + e) % zl;
                            wlines[g].insert(off + e - in_pos % RFT_LINE);
                        }
                    }
    for (int g = 0; g < RFT_KGROUPS; ++g)
        if (tlines[g] != wlines[g]) fail("k-group's touched lines differ from the lines its walk reads", g, (long long)tlines[g].size(), (long long)wlines[g].size());
    if ((long long)floats.size() != (long long)L * RFT_CH) fail("the walk does not read every float of the row", (long long)floats.size(), L, 0);
    for (auto& kv : floats)
        if (kv.second != 1) fail("float read more than once", kv.first, kv.second, 0);
    printf("L=%d zl=%lld: %zu lines touched, %zu floats walked, %d failures\n", L, zl, touched.size(), floats.size(), bad);
    return bad ? 1 : 0;
}
