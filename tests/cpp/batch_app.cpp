// batch_app.cpp -- a caller of the batched decode through the drop-in include/rwkv.h: prefill one prompt, fork it into N state
// slots, continue the N streams on the device.  Used by tests/test_batch_decode_cpu.py.
//   batch_app <model.bin> <n_streams> <n_steps>   -> one line of n_steps greedy ids per stream (stream s fed 100 + s after the
//                                                    fork), then one line per stream of typical ids (seed s), then "batch_ok"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rwkv.h"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const unsigned long long n = strtoull(argv[2], nullptr, 10), steps = strtoull(argv[3], nullptr, 10);
    RWKV model;
    try { model.decodeBatchGreedy({1, 2}, 1); return 3; } catch (const std::runtime_error &) {}
    model.loadFile(argv[1], n);
    model.loadContext(std::vector<long long>{5, 6, 7});          // prefill on slot 0 (host-authoritative mode)
    for (unsigned long long s = 1; s < n; s++) model.copyState(s, 0);
    std::vector<unsigned long long> first(n), seeds(n);
    for (unsigned long long s = 0; s < n; s++) { first[s] = 100 + s; seeds[s] = s; }
    RWKVState snap = *model.state;
    const std::vector<unsigned long long> g = model.decodeBatchGreedy(first, steps);
    *model.state = snap;
    const std::vector<unsigned long long> t = model.decodeBatchTypical(first, steps, seeds, 0.9f, 0.8f);
    for (const auto *ids : {&g, &t})
        for (unsigned long long s = 0; s < n; s++) {
            for (unsigned long long k = 0; k < steps; k++) printf("%llu ", (*ids)[s * steps + k]);
            printf("\n");
        }
    try { model.decodeBatchGreedy(std::vector<unsigned long long>(n + 1, 1), 1); return 4; } catch (const std::runtime_error &) {}
    printf("batch_ok\n");
    return 0;
}
