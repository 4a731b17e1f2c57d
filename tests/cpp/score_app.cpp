// score_app.cpp -- a caller of the device scorer through the drop-in include/rwkv.h: score a document, then the rows a forward left.
// Used by tests/test_score_api_cpu.py (compiles and links without a GPU) and tests/test_score_gpu.py (runs).
//   score_app <model.bin> <max_ctx> <id> <id> ...   -> one line "%.17g" per log-probability of ids[1:] (RWKV::score), then one line
//                                                      per log-probability, entropy and argmax of RWKV::scoreRows on the rows the
//                                                      last piece left (row r against target ids[r]), then "score_ok"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rwkv.h"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const unsigned long long max_ctx = strtoull(argv[2], nullptr, 10);
    std::vector<unsigned long long> doc;
    for (int i = 3; i < argc; i++) doc.push_back(strtoull(argv[i], nullptr, 10));
    RWKV model;
    try { model.score(doc); return 3; } catch (const std::runtime_error &) {}
    try { model.scoreRows({0}, {1}); return 3; } catch (const std::runtime_error &) {}
    model.loadFile(argv[1], max_ctx);
    const RWKV::Scores s = model.score(doc);
    if (s.logprob.size() != doc.size() - 1 || s.entropy.size() != s.logprob.size() || s.argmax.size() != s.logprob.size()) return 4;
    for (double v : s.logprob) printf("%.17g\n", v);
    // the last piece's rows: (doc.size() - 1) % max_ctx of them, or max_ctx when that is 0
    const size_t fed = doc.size() - 1, rows = fed % max_ctx ? fed % max_ctx : (size_t)max_ctx;
    std::vector<unsigned long long> r, g;
    for (size_t i = 0; i < rows; i++) { r.push_back(i); g.push_back(doc[i]); }
    const RWKV::Scores q = model.scoreRows(r, g);
    for (size_t i = 0; i < rows; i++) printf("%.17g %.17g %llu\n", q.logprob[i], q.entropy[i], q.argmax[i]);
    try { model.scoreRows({max_ctx}, {1}); return 5; } catch (const std::runtime_error &) {}
    try { model.score({1, 2}, {3, RWKV_VOCAB}); return 5; } catch (const std::runtime_error &) {}
    printf("score_ok\n");
    return 0;
}
