// logprobs_app.cpp -- a caller of rwkv_decode_batch_logprobs and rwkv_topn_rows through the drop-in include/rwkv.h: prefill one prompt, fork it
// into N state slots, continue the N streams with the nucleus sampler and penalties, and report what the model thought of every generated token.
// Used by tests/test_logprobs_cpu.py (compiles and links without a GPU) and tests/test_logprobs_gpu.py (runs).
//   logprobs_app <model.bin> <n_streams> <n_steps> <top_n>
//     -> per stream and step one line "s k id logprob entropy  id_0 lp_0 .. id_{top_n-1} lp_{top_n-1}" (stream s fed 100 + s after the fork,
//        seed s; every double as %a, so that a caller can compare bit for bit), then per stream one line "row s  id_0 lp_0 .." with
//        RWKV::topnRows of the logits rows the last step left, then "logprobs_ok"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rwkv.h"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const unsigned long long n = strtoull(argv[2], nullptr, 10), steps = strtoull(argv[3], nullptr, 10);
    const unsigned top_n = (unsigned)strtoul(argv[4], nullptr, 10);
    RWKV model;
    try { model.decodeBatchLogprobs({1, 2}, 1, RWKV::Pick::greedy(), {}, RWKV::Stop{}, 1); return 3; } catch (const std::runtime_error &) {}
    try { model.topnRows({0}, 1); return 3; } catch (const std::runtime_error &) {}
    model.loadFile(argv[1], n);
    model.loadContext(std::vector<long long>{5, 6, 7});          // prefill on slot 0 (host-authoritative mode)
    for (unsigned long long s = 1; s < n; s++) model.copyState(s, 0);
    std::vector<unsigned long long> first(n), seeds(n), rows(n);
    for (unsigned long long s = 0; s < n; s++) { first[s] = 100 + s; seeds[s] = s; rows[s] = s; }
    const RWKV::Logprobs r = model.decodeBatchLogprobs(first, steps, RWKV::Pick::nucleus(RWKV::Nucleus{1.0f, 0.9f, 0, 0.4f, 0.4f, 0.996f}), seeds,
                                                       RWKV::Stop{}, top_n);
    if (r.until.ids.size() != n * steps || r.logprob.size() != n * steps || r.entropy.size() != n * steps || r.top_n != top_n ||
        r.top_ids.size() != n * steps * top_n || r.top_logprob.size() != r.top_ids.size())
        return 4;
    for (unsigned long long s = 0; s < n; s++)
        for (unsigned long long k = 0; k < steps; k++) {
            const size_t at = s * steps + k;
            printf("%llu %llu %llu %a %a ", s, k, r.until.ids[at], r.logprob[at], r.entropy[at]);
            for (unsigned j = 0; j < top_n; j++) printf(" %llu %a", r.top_ids[at * top_n + j], r.top_logprob[at * top_n + j]);
            printf("\n");
        }
    if (top_n) {
        const RWKV::TopN t = model.topnRows(rows, top_n);
        if (t.ids.size() != n * top_n || t.logprob.size() != n * top_n) return 4;
        for (unsigned long long s = 0; s < n; s++) {
            printf("row %llu ", s);
            for (unsigned j = 0; j < top_n; j++) printf(" %llu %a", t.ids[s * top_n + j], t.logprob[s * top_n + j]);
            printf("\n");
        }
        try { model.topnRows({n}, top_n); return 5; } catch (const std::runtime_error &) {}
        try { model.topnRows(rows, RWKV_MAX_TOPN + 1); return 5; } catch (const std::runtime_error &) {}
    }
    try { model.decodeBatchLogprobs(first, steps, RWKV::Pick::greedy(), {}, RWKV::Stop{}, RWKV_MAX_TOPN + 1); return 5; } catch (const std::runtime_error &) {}
    printf("logprobs_ok\n");
    return 0;
}
