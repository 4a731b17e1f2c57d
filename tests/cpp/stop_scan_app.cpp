// host stop-scan check: runs stop_scan() of include/rwkv_sampler.h over the cases of a text file.  Used by tests/test_stop_cpu.py.
//   stop_scan_app cases.txt     one case per record of whitespace-separated integers:
//        first  max_new (0: none)  n_hist hist...  n_ids ids...  n_stops { len ids... }
//   -> per case one line: len reason n_hist hist...
#include <cstdio>
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

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 3;
    unsigned long long first = 0, max_new = 0, n_stops = 0;
    while (fscanf(f, "%llu %llu", &first, &max_new) == 2) {
        std::vector<unsigned long long> history, ids;
        if (!read_list(f, history) || !read_list(f, ids) || fscanf(f, "%llu", &n_stops) != 1 || n_stops > 16) return 4;
        std::vector<std::vector<unsigned long long>> stops(n_stops);
        for (auto &q : stops)
            if (!read_list(f, q)) return 4;
        const stop_result r = stop_scan(ids, first, stops, (unsigned)max_new, history);
        printf("%u %u %zu", r.len, r.reason, history.size());
        for (unsigned long long h : history) printf(" %llu", h);
        printf("\n");
    }
    fclose(f);
    return 0;
}
