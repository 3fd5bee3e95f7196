// Host check of csrc/grid_map.h (compiled and run by test_grid_map_host.py): for a grid of nwg workgroups,
//   - bid -> xcd_contiguous(bid, nwg) is a permutation of 0 .. nwg - 1;
//   - the blocks of XCD x (bid & 7 == x), in launch order, take one contiguous ascending range;
//   - the ranges follow each other in the order of x, starting at 0, and their sizes differ by at most one.
// usage: grid_map_host N | LO-HI ...      (prints one line, exit status 0 = all checks hold for every grid size given)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "grid_map.h"

static int bad = 0;
static void fail(const char* what, unsigned nwg, unsigned a, unsigned b) {
    if (bad++ < 10) fprintf(stderr, "nwg=%u: %s (%u, %u)\n", nwg, what, a, b);
}

static void check(unsigned nwg) {
    std::vector<unsigned char> seen(nwg, 0);
    unsigned next = 0, lo = nwg, hi = 0;                                   // next: where the range of the next XCD must start
    for (unsigned x = 0; x < 8; ++x) {
        unsigned size = 0;
        for (unsigned bid = x; bid < nwg; bid += 8, ++size) {
            const unsigned w = xcd_contiguous(bid, nwg);
            if (w >= nwg) { fail("image outside the grid", nwg, bid, w); continue; }
            if (seen[w]++) fail("image produced twice", nwg, bid, w);
            if (w != next + size) fail("XCD's images not one ascending range behind the previous XCD's", nwg, bid, w);
        }
        next += size;
        if (size < lo) lo = size;
        if (size > hi) hi = size;
    }
    if (next != nwg) fail("ranges do not cover the grid", nwg, next, 0);
    for (unsigned w = 0; w < nwg; ++w)
        if (!seen[w]) { fail("item without a block", nwg, w, 0); break; }
    if (hi - lo > 1) fail("range sizes differ by more than one", nwg, lo, hi);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    unsigned long long grids = 0;
    for (int i = 1; i < argc; ++i) {
        const char* dash = strchr(argv[i], '-');
        const long long a = atoll(argv[i]), b = dash ? atoll(dash + 1) : a;
        if (a < 1 || b < a || b >= (1LL << 31)) return 2;
        for (long long n = a; n <= b; ++n, ++grids) check((unsigned)n);
    }
    printf("%llu grid sizes, %d failures\n", grids, bad);
    return bad ? 1 : 0;
}
