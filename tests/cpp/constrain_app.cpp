// constrain_app.cpp -- a caller of rwkv_constraint_set, rwkv_decode_batch_constrained and rwkv_pick_constrained through the drop-in include/rwkv.h:
// the multiple-choice recipe.  Prefill one prompt, fork it into N state slots, build the automaton of four answers with constraint_trie
// (include/rwkv_sampler.h), and let every stream spell one of them -- greedily, then with the nucleus sampler, penalties and a logit bias that bans
// the first token of one answer.
// Used by tests/test_constraint_cpu.py (compiles and links without a GPU) and tests/test_constraint_gpu.py (runs).
//   constrain_app <model.bin> <n_streams> <n_steps>
//     -> per run ("greedy", "nucleus") and stream one line "run s len reason state  id_0 .. id_{n_steps-1}" (stream s fed 100 + s after the fork,
//        seed s), then one line "pick token state" of a single constrained greedy draw from row 0 in state 0, then "constrain_ok"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rwkv.h"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const unsigned long long n = strtoull(argv[2], nullptr, 10), steps = strtoull(argv[3], nullptr, 10);
    const std::vector<std::vector<unsigned long long>> choices = {{100, 200}, {100, 201, 300}, {100, 201, 301}, {5000, 6000, 7000, 8000}};
    const constraint_automaton trie = constraint_trie(choices);
    const RWKV::Automaton automaton{trie.row_ptr, trie.tok, trie.next};
    RWKV model;
    try { model.setConstraint(automaton); return 3; } catch (const std::runtime_error &) {}      // not loaded
    model.loadFile(argv[1], n);
    model.loadContext(std::vector<long long>{5, 6, 7});          // prefill on slot 0 (host-authoritative mode)
    for (unsigned long long s = 1; s < n; s++) model.copyState(s, 0);
    try { model.setConstraint(RWKV::Automaton{{0, 1}, {0}, {0}}); return 4; } catch (const std::runtime_error &) {}      // an edge on id 0
    model.setConstraint(automaton);
    std::vector<unsigned long long> first(n), seeds(n);
    for (unsigned long long s = 0; s < n; s++) { first[s] = 100 + s; seeds[s] = s; }
    const std::vector<unsigned> start(n, 0u);
    std::vector<RWKV::Bias> bias(n);
    bias[0] = RWKV::Bias{{100}, {-INFINITY}};                    // stream 0 may not begin with 100: it spells the fourth answer
    for (int run = 0; run < 2; run++) {
        const RWKV::Pick pick = run ? RWKV::Pick::nucleus(RWKV::Nucleus{1.0f, 0.9f, 0, 0.4f, 0.4f, 0.996f}) : RWKV::Pick::greedy();
        const RWKV::Constrained r = model.decodeConstrained(first, steps, pick, seeds, RWKV::Stop{}, start, run ? bias : std::vector<RWKV::Bias>{});
        if (r.until.ids.size() != n * steps || r.until.len.size() != n || r.until.reason.size() != n || r.state.size() != n) return 5;
        for (unsigned long long s = 0; s < n; s++) {
            printf("%s %llu %u %u %u ", run ? "nucleus" : "greedy", s, r.until.len[s], r.until.reason[s], r.state[s]);
            for (unsigned long long k = 0; k < steps; k++) printf(" %llu", r.until.ids[s * steps + k]);
            printf("\n");
        }
    }
    try { model.decodeConstrained(first, steps, RWKV::Pick::typical(), seeds, RWKV::Stop{}, start); return 6; } catch (const std::runtime_error &) {}
    try { model.decodeConstrained(first, steps, RWKV::Pick::greedy(), seeds); return 6; } catch (const std::runtime_error &) {}      // the slots stand on leaves
    model.forward(first[0]);
    const std::vector<unsigned> zero(1, 0u);
    if (rwkv_constraint_state_set(model.handle(), 0, 1, zero.data()) != 0) return 7;
    const std::pair<unsigned long long, unsigned> p = model.pickConstrained(RWKV::Pick::greedy());
    printf("pick %llu %u\n", p.first, p.second);
    model.clearConstraint();
    printf("constrain_ok\n");
    return 0;
}
