// Stand-alone check of sell_find_period (csrc/sell_period.cpp) for a sanitizer build: the host function on synthetic records and
// lists of the kinds tests/test_sell_period_cpu.py uses, no device and no Python.
//
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Iaocl-sparse_amd/csrc tools/sell_period_check.cpp aocl-sparse_amd/csrc/sell_period.cpp -o tools/bin/sell_period_check
//   tools/bin/sell_period_check        (prints one line per case; exit status 0 when every case has the expected range)
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

// n slices repeating `period` distinct ones: mode 1, width 5, the word in the record, lists moving by 64 per slice
Arrays pattern(int n, int period)
{
    Arrays a;
    a.rec.resize((size_t)n), a.lists.assign((size_t)n * SELL_SHORT_WMAX, -1);
    for(int s = 0; s < n; s++)
    {
        const int ph = s % period;
        a.rec[(size_t)s] = {0x10u + (unsigned)ph, 0x9e3779b9u * (unsigned)s, (0x7f4a7c15u * (unsigned)s) << 16,
                            5u | 1u << 8 | (unsigned)SELL_DESC_MODE_LANE_SHIFT << 16 | SELL_DESC_UWORD};
        for(int q = 0; q < 5; q++)
            a.lists[(size_t)s * SELL_SHORT_WMAX + q] = 1000 + 64 * s + 7 * q + (ph * (q + 1)) % 7;
    }
    return a;
}

int failures = 0;

void expect(const char *what, const Arrays &a, int cap, int lo, int hi, int per)
{
    aoclsparse_int out[4] = {-1, -1, -1, -1};
    sell_find_period(a.rec.data(), a.lists.data(), (aoclsparse_int)a.rec.size(), cap, out);
    const bool ok = out[0] == lo && out[1] == hi && out[2] == per && out[3] == 64 * per;
    std::printf("%-44s {%d, %d, %d, %d} %s\n", what, (int)out[0], (int)out[1], (int)out[2], (int)out[3], ok ? "ok" : "WRONG");
    failures += !ok;
}
} // namespace

int main()
{
    expect("one pattern of 12 slices", pattern(256, 12), 64, 0, 256, 12);
    expect("period 1 -> 4", pattern(240, 1), 64, 0, 240, 4);
    expect("period 5 -> 20", pattern(240, 5), 64, 0, 240, 20);
    expect("257 slices", pattern(257, 12), 64, 0, 256, 12);
    expect("7 slices: nothing", pattern(7, 4), 64, 0, 0, 0);
    expect("8 slices, two periods", pattern(8, 4), 64, 0, 8, 4);
    expect("period above the cap", pattern(400, 68), 64, 0, 0, 0);
    expect("cap of 3", pattern(400, 4), 3, 0, 0, 0);
    {
        Arrays a = pattern(400, 8);
        a.lists[101 * SELL_SHORT_WMAX + 4] += 1;
        expect("a column of slice 101 differs", a, 64, 104, 400, 8);
        a = pattern(400, 8);
        a.rec[101].wsm = 5u | 3u << 8 | (unsigned)SELL_DESC_MODE_OWN << 16;
        expect("slice 101 reads the lists in col", a, 64, 104, 400, 8);
        a = pattern(400, 8);
        for(int s = 0; s < 21; s++)
            a.lists[(size_t)s * SELL_SHORT_WMAX] += 7;
        for(int s = 390; s < 400; s++)
            a.lists[(size_t)s * SELL_SHORT_WMAX + 1] -= 1;
        expect("head and tail that do not repeat", a, 64, 24, 388, 8);
        a = pattern(400, 8);
        for(int s = 40; s < 400; s += 8)
            a.rec[(size_t)s].wsm = 0u | 1u << 8 | (unsigned)SELL_DESC_MODE_ONE << 16;
        expect("slices of width 0", a, 64, 0, 0, 0);
        a = pattern(400, 8);
        for(int s = 190; s < 400; s++)
            a.lists[(size_t)s * SELL_SHORT_WMAX + 2] += s * s;
        expect("a range under half", a, 64, 0, 0, 0);
    }
    {
        // a grid line of 64 slices between two lines that differ, exception slices at the ends of every line
        Arrays a = pattern(64 * 40, 1);
        for(int s = 0; s < 64 * 40; s++)
        {
            if(s % 64 == 0 || s % 64 == 63)
            {
                a.rec[(size_t)s].wsm     = 5u | 2u << 8 | SELL_DESC_UWORD | SELL_DESC_EXCEPT;
                a.rec[(size_t)s].cell_lo = 0x15u | (s % 64 ? 63u : 0u) << 8 | 0x1du << 16 | 0xffu << 24;
                a.rec[(size_t)s].hi      = (a.rec[(size_t)s].hi & 0xffff0000u) | 0x1fu;
            }
            if(s < 64 || s >= 64 * 39)
                a.rec[(size_t)s].wsm = (a.rec[(size_t)s].wsm & ~0xffu) | 4u;
        }
        expect("40 grid lines of 64 slices", a, 4096, 64, 64 * 39, 64);
    }
    {
        // 40 % of the slices, around the centre, repeat with every period; the rest is eligible and repeats with none: the search
        // gives up within its budget
        Arrays a = pattern(20000, 1);
        for(int s = 0; s < 20000; s++)
            if(s < 6000 || s >= 14000)
                a.lists[(size_t)s * SELL_SHORT_WMAX + 2] += (s * 7919) % 1009 + s;
        expect("a stencil embedded in noise", a, 4096, 0, 0, 0);
        aoclsparse_int out[4];
        long long      work = -1;
        sell_find_period(a.rec.data(), a.lists.data(), 20000, 4096, out, &work);
        std::printf("%-44s %lld comparisons for 20000 slices %s\n", "", work, work <= 8LL * 20000 ? "ok" : "WRONG");
        failures += !(work <= 8LL * 20000);
    }
    std::printf("%d failure(s)\n", failures);
    return failures != 0;
}
