// stop_app.cpp -- a caller of rwkv_decode_batch_until through the drop-in include/rwkv.h: prefill one prompt, fork it into N state slots,
// continue the N streams with the nucleus sampler until each one's budget or the stop sequence.  Used by tests/test_stop_gpu.py.
//   stop_app <model.bin> <n_streams> <n_steps> <budget per stream ...> -- <stop sequence ids ...>
//     -> per stream one line "len reason id_0 .. id_{n_steps-1}" (stream s fed 100 + s after the fork, seed s), then "stop_ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rwkv.h"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const unsigned long long n = strtoull(argv[2], nullptr, 10), steps = strtoull(argv[3], nullptr, 10);
    RWKV::Stop stop;
    int i = 4;
    for (; i < argc && strcmp(argv[i], "--"); i++) stop.max_new.push_back((unsigned)strtoul(argv[i], nullptr, 10));
    stop.sequences.emplace_back();
    for (i++; i < argc; i++) stop.sequences[0].push_back(strtoull(argv[i], nullptr, 10));
    if (stop.max_new.size() != n || stop.sequences[0].empty()) return 2;
    RWKV model;
    try { model.decodeBatchUntil({1, 2}, 1, RWKV::Pick::greedy(), {}, stop); return 3; } catch (const std::runtime_error &) {}
    model.loadFile(argv[1], n);
    model.loadContext(std::vector<long long>{5, 6, 7});          // prefill on slot 0 (host-authoritative mode)
    for (unsigned long long s = 1; s < n; s++) model.copyState(s, 0);
    std::vector<unsigned long long> first(n), seeds(n);
    for (unsigned long long s = 0; s < n; s++) { first[s] = 100 + s; seeds[s] = s; }
    const RWKV::Until r = model.decodeBatchUntil(first, steps, RWKV::Pick::nucleus(RWKV::Nucleus{1.0f, 0.9f, 0, 0.4f, 0.4f, 0.996f}), seeds, stop);
    if (r.steps_run == 0 || r.steps_run > steps) return 4;
    for (unsigned long long s = 0; s < n; s++) {
        printf("%u %u", r.len[s], r.reason[s]);
        for (unsigned long long k = 0; k < steps; k++) printf(" %llu", r.ids[s * steps + k]);
        printf("\n");
    }
    RWKV::Stop bad = stop;
    bad.sequences[0].assign(9, 1);                               // longer than RWKV_STOP_MAX_LEN
    try { model.decodeBatchUntil(first, steps, RWKV::Pick::greedy(), {}, bad); return 5; } catch (const std::runtime_error &) {}
    printf("stop_ok\n");
    return 0;
}
