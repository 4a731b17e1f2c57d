// host DRY check: runs dry_scan() and dry_table() of include/rwkv_sampler.h over the cases of a text file.  Used by tests/test_dry_cpu.py.
//   dry_app cases.txt     one case per record of whitespace-separated integers:  allowed window  n_breakers breakers...  n_ids ids...
//   -> per case one line: the (id, L) pairs flattened;  last line: "table" and the bit patterns of dry_table(0.8, 1.75)[0, 1, 63] and of
//      dry_table(inf, 1.75)[63]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rwkv_sampler.h"

static bool read_list(FILE *f, std::vector<unsigned long long> &v)
{
    unsigned long long n = 0;
    if (fscanf(f, "%llu", &n) != 1 || n > 65536) return false;
    v.resize(n);
    for (auto &x : v)
        if (fscanf(f, "%llu", &x) != 1) return false;
    return true;
}

static unsigned bits(float v) { unsigned b; std::memcpy(&b, &v, 4); return b; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 3;
    unsigned allowed = 0, window = 0;
    while (fscanf(f, "%u %u", &allowed, &window) == 2) {
        std::vector<unsigned long long> br, ids;
        if (!read_list(f, br) || !read_list(f, ids)) return 4;
        for (const dry_hit &h : dry_scan(ids, allowed, window, std::vector<unsigned>(br.begin(), br.end()))) printf("%u %u ", h.id, h.len);
        printf("\n");
    }
    fclose(f);
    const std::vector<float> a = dry_table(0.8f, 1.75f), b = dry_table(INFINITY, 1.75f);
    printf("table %u %u %u %u\n", bits(a[0]), bits(a[1]), bits(a[63]), bits(b[63]));
    return 0;
}
