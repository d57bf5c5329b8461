// Stand-alone check of sell_find_march (csrc/sell_period.cpp) and sell_march_rule (csrc/internal.hpp) for a sanitizer build: the host
// functions on synthetic records and lists of the kinds tests/test_sell_march_cpu.py uses, the arrays allocated EXACTLY (a read
// beyond the first period's slices or beyond a list's eight entries is a finding), no device and no Python.
//
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Iaocl-sparse_amd/csrc tools/sell_march_check.cpp aocl-sparse_amd/csrc/sell_period.cpp -o tools/bin/sell_march_check
//   tools/bin/sell_march_check        (prints one line per case; exit status 0 when every case has the expected result)
#include "internal.hpp"

#include <cstdio>
#include <vector>

using namespace mi355;

namespace
{
struct Arrays
{
    std::vector<SellSliceDesc>  rec;
    std::vector<aoclsparse_int> lists;
};

// n slices of rows r + offs[q]: mode 1, the word in the record
Arrays stencil(int n, const std::vector<int> &offs)
{
    Arrays a;
    a.rec.resize((size_t)n), a.lists.assign((size_t)n * SELL_SHORT_WMAX, -1);
    for(int s = 0; s < n; s++)
    {
        a.rec[(size_t)s] = {0x15u, 0u, 0u, (unsigned)offs.size() | 64u << 8 | (unsigned)SELL_DESC_MODE_LANE_SHIFT << 16 | SELL_DESC_UWORD};
        for(size_t q = 0; q < offs.size(); q++)
            a.lists[(size_t)s * SELL_SHORT_WMAX + q] = 64 * s + offs[q];
    }
    return a;
}

int failures = 0;

void expect(const char *what, const Arrays &a, aoclsparse_int lo, aoclsparse_int hi, aoclsparse_int per, aoclsparse_int stride, int bytes,
            int stack, unsigned map)
{
    const aoclsparse_int range[4] = {lo, hi, per, stride};
    aoclsparse_int       out[2]   = {-1, -1};
    sell_find_march(a.rec.data(), a.lists.data(), (aoclsparse_int)a.rec.size(), range, bytes, out);
    const bool ok = out[0] == stack && (unsigned)out[1] == map;
    std::printf("%-52s {%d, 0x%x} %s\n", what, (int)out[0], (unsigned)out[1], ok ? "ok" : "WRONG");
    failures += !ok;
}

void expect_rule(const char *what, aoclsparse_int n, int lo, int hi, int per, int elo, int ehi, int eg)
{
    const SellMarch r  = sell_march_rule(n, 5, lo, hi, per, 64 * per, 1, 0x503u, 8, SELL_MARCH_SPW);
    const bool      ok = r.lo == elo && r.hi == ehi && r.g == eg && r.alias == (eg ? 0x503u : 0u);
    std::printf("%-52s {%d, %d, %d, 0x%x} %s\n", what, r.lo, r.hi, r.g, r.alias, ok ? "ok" : "WRONG");
    failures += !ok;
}
} // namespace

int main()
{
    const std::vector<int> five = {0, 255, 256, 257, 512}, seven = {0, 3840, 4095, 4096, 4097, 4352, 8192};
    expect("5 cells, the range is the whole array", stencil(64, five), 0, 64, 4, 256, 1, 1, 0x503u);
    expect("7 cells", stencil(64, seven), 0, 64, 4, 256, 1, 1, 0x6040u);
    expect("8 cells, the first period ends the array", stencil(8, {0, 1, 2, 3, 256, 257, 258, 259}), 4, 8, 4, 256, 1, 1, 0x8765u);
    expect("a period of 16 slices: no alias", stencil(64, five), 16, 64, 16, 1024, 1, 1, 0u);
    expect("two-byte words", stencil(64, five), 0, 64, 4, 256, 2, 0, 0x503u);
    {
        Arrays a = stencil(64, five);
        a.lists[2 * SELL_SHORT_WMAX + 1] += 1;
        expect("a list that does not continue the group's first", a, 0, 64, 4, 256, 1, 0, 0x503u);
        a = stencil(64, five);
        a.rec[3].wsm &= ~SELL_DESC_UWORD;
        expect("a slice without its word", a, 0, 64, 4, 256, 1, 0, 0x503u);
        a = stencil(64, five);
        for(int s = 0; s < 64; s++)
            a.lists[(size_t)s * SELL_SHORT_WMAX + 4] = -1;
        expect("an unused entry inside the width", a, 0, 64, 4, 256, 1, 0, 0x3u);
        a = stencil(64, five);
        a.lists[1 * SELL_SHORT_WMAX + 4] += 1;
        expect("an alias that fails in one slice", a, 0, 64, 4, 256, 1, 0, 0x3u);
        a = stencil(64, five);
        a.rec[0].wsm = (a.rec[0].wsm & ~0xff0000u) | SELL_DESC_EXCEPT;
        expect("an exception slice counts as shifted", a, 0, 64, 4, 256, 1, 1, 0x503u);
    }
    expect("a range beyond the array", stencil(64, five), 0, 68, 4, 256, 1, 0, 0u);
    expect("a period that is no multiple of 4", stencil(64, five), 0, 64, 6, 384, 1, 0, 0u);
    expect("a range shorter than its period", stencil(64, five), 60, 64, 8, 512, 1, 0, 0u);
    expect_rule("the headline: 4094 periods of 64", 262144, 64, 262080, 64, 64, 64 + 4092 * 64, 3);
    expect_rule("15,358 periods of 4: whole workgroups", 61440, 4, 61436, 4, 4, 4 + 5118 * 3 * 4, 3);
    expect_rule("five periods of 4: one group is no workgroup", 4096, 16, 36, 4, 0, 0, 0);
    expect_rule("two periods", 4096, 16, 24, 4, 0, 0, 0);
    std::printf("%d failure(s)\n", failures);
    return failures != 0;
}
