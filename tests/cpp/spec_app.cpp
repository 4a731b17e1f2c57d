// spec_app.cpp -- a caller of rwkv_spec_verify and rwkv_decode_speculative through the drop-in include/rwkv.h: prefill one prompt on slot 0 of a
// target and of a draft model, and continue it greedily with the draft model guessing and the target verifying.  Used by tests/test_spec_cpu.py
// (compiles and links without a GPU) and tests/test_spec_gpu.py (runs).
//   spec_app <target.bin> <draft.bin> <n_tokens> <k>
//     -> "ids id_0 .. id_{n-1}" (fed 100 behind the prompt 5 6 7), "stats rounds drafted accepted", then "verify a next" of one more
//        specVerify with a draft made of the two ids a second decodeSpeculative emits first, then "spec_ok"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rwkv.h"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const unsigned long long n = strtoull(argv[3], nullptr, 10);
    const unsigned k = (unsigned)strtoul(argv[4], nullptr, 10);
    RWKV model, draft;
    try { model.specVerify(100, {}); return 3; } catch (const std::runtime_error &) {}
    try { model.decodeSpeculative(draft, 100, n, k); return 3; } catch (const std::runtime_error &) {}
    model.loadFile(argv[1], k + 2);
    draft.loadFile(argv[2], k + 2);
    const std::vector<long long> prompt{5, 6, 7};
    model.loadContext(prompt);                                    // prefill on slot 0 (host-authoritative mode), of both
    draft.loadContext(prompt);
    const RWKV::SpecResult r = model.decodeSpeculative(draft, 100, n, k);
    if (r.tokens.size() != n || r.accepted > r.drafted || r.rounds == 0 || r.rounds > n) return 4;
    printf("ids");
    for (unsigned long long t : r.tokens) printf(" %llu", t);
    printf("\nstats %llu %llu %llu\n", r.rounds, r.drafted, r.accepted);
    // the call chains: its last id is the next call's first; a draft made of what follows is accepted whole by a verify from the same state
    const RWKVState before = *model.state;
    const RWKV::SpecResult more = model.decodeSpeculative(draft, r.tokens.back(), 3, k);
    *model.state = before;
    const RWKV::SpecStep s = model.specVerify(r.tokens.back(), {more.tokens[0], more.tokens[1]});
    printf("verify %llu %llu\n", s.accepted, s.next);
    if (s.accepted != 2 || s.next != more.tokens[2]) return 5;
    try { model.specVerify(100, std::vector<unsigned long long>(RWKV_SPEC_MAX_DRAFT + 1, 5)); return 6; } catch (const std::runtime_error &) {}
    try { model.decodeSpeculative(model, 100, n, k); return 6; } catch (const std::runtime_error &) {}
    try { model.decodeSpeculative(draft, 100, n, 0); return 6; } catch (const std::runtime_error &) {}
    printf("spec_ok\n");
    return 0;
}
