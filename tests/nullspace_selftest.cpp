// Stand-alone check of the index work of the null-space basis (restab::null_* of csrc/stmmqr_restables.cpp; tests/test_nullspace_cpu.py
// builds both with g++ under ASan + UBSan): the split into live and dead columns, the slab partition of the rows of N, the panels of
// the Cholesky factorization and the tiles of the Gram matrix, against values written out here or recomputed by brute force.
#include <cstdio>
#include <vector>

#include "stmmqr_restables.h"

using namespace restab;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_split()
{
    std::vector<int> pc = {9}, jd = {9};
    null_split({}, pc, jd);
    CHECK(pc.empty() && jd.empty(), "no column");
    null_split({0, 1, 0, 0, 1, 1, 0}, pc, jd);
    CHECK((pc == std::vector<int>{0, 2, 3, 6}), "live");
    CHECK((jd == std::vector<int>{1, 4, 5}), "dead");
    null_split({1, 1}, pc, jd);
    CHECK(pc.empty() && (jd == std::vector<int>{0, 1}), "rank zero");
    null_split({0, 0, 2}, pc, jd);                       // (any non-zero flag is dead)
    CHECK(pc.size() == 2 && (jd == std::vector<int>{2}), "flag 2");
}

// every row in exactly one slab, slabs in order, none empty, none above the height
static void check_slabs()
{
    const long ncols[] = {0, 1, 63, 64, 65, 127, 129, 2047, 2048, 2049, 17500, 1L << 22, (1L << 31) - 1};
    const long wants[] = {-5, 0, 1, 16, 64, 2048, 1L << 20};
    for (long ncol : ncols)
        for (long want : wants) {
            const NullSlabs s = null_slabs(ncol, want);
            CHECK(s.height >= 1 && s.height >= want, "ncol %ld want %ld: height %d", ncol, want, s.height);
            CHECK(s.count >= 1 && s.count <= 65535, "ncol %ld want %ld: count %d", ncol, want, s.count);
            CHECK((long)s.height * s.count >= ncol, "ncol %ld want %ld: the slabs end at row %ld", ncol, want, (long)s.height * s.count);
            CHECK(ncol == 0 || (long)s.height * (s.count - 1) < ncol, "ncol %ld want %ld: an empty slab", ncol, want);
            if ((ncol + std::max(1L, want) - 1) / std::max(1L, want) <= 65535)
                CHECK(s.height == std::max(1L, want), "ncol %ld want %ld: height %d was raised without need", ncol, want, s.height);
        }
    CHECK(null_slabs(65, 64).count == 2 && null_slabs(63, 64).count == 1 && null_slabs(128, 64).count == 2, "the slab edges");
    CHECK(null_slabs(1L << 22, 1).height == 128, "4 Mi rows in slabs of 1: raised to 128 (32768 slabs)");
}

static void check_panels()
{
    CHECK(null_panels(0) == 0 && null_panels(1) == 1 && null_panels(31) == 1 && null_panels(32) == 1 && null_panels(33) == 2 &&
          null_panels(64) == 2 && null_panels(496) == 16 && null_panels(2086) == 66, "panel counts");
    const int ds[] = {1, 31, 32, 33, 64, 496, 2086};
    for (int d : ds) {
        int total = 0;
        for (int p = 0; p < null_panels(d); p++) {
            const int w = null_panel_width(d, p);
            CHECK(w >= 1 && w <= STM_NULL_NB && (w == STM_NULL_NB || p == null_panels(d) - 1), "d %d panel %d: width %d", d, p, w);
            total += w;
        }
        CHECK(total == d && null_panel_width(d, null_panels(d)) == 0, "d %d: the panels hold %d columns", d, total);
        long long tiles = 0;
        for (int ti = 0; ti < null_panels(d); ti++)
            for (int tj = 0; tj <= ti; tj++) {
                CHECK((long long)ti * (ti + 1) / 2 + tj == tiles, "d %d: tile (%d, %d) is not number %lld", d, ti, tj, tiles);   // the kernels' numbering
                tiles++;
            }
        CHECK(tiles == null_lower_tiles(d), "d %d: %lld lower tiles, not %lld", d, null_lower_tiles(d), tiles);
    }
    CHECK(null_panel_width(496, 15) == 16 && null_panel_width(2086, 65) == 6, "the narrow last panels of dwt_992 and lns_3937");
    CHECK(null_lower_tiles(46341 * 32) == 46341LL * 46342 / 2, "beyond 2^31 partial-tile doubles per slab");
}

int main()
{
    check_split();
    check_slabs();
    check_panels();
    printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures != 0;
}
