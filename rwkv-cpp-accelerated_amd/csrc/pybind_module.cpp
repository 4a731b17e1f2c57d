// pybind_module.cpp -- the reference's pybind module `rwkv` (bindings/pybind/c_binding.cpp:158-175)
// on top of this repo's include/rwkv.h: same function names, arguments and return shapes, so
// bindings/pybind/binding.py (ModelWrapper) works unchanged with SO_LIB_PATH pointing at it.
//
//   initRwkv() -> handle            loadModel(h, path) -> (n_layers, n_embed)
//   modelForward(h, token)          initState(h) / getState(h) -> [5 x np.float64]
//   initOutput(h) / getOutput(h) -> np.float32[50277]        typicalSample(h, temp, tau) -> int
//
// Deliberate fixes of reference quirks:
//   * initState really zeroes the state forward() uses (the reference re-allocates only the
//     deprecated alias pointers, c_binding.cpp:41-60); getState returns the L*D state (the
//     reference copies 50277 elements from those aliases, c_binding.cpp:104-110).
//   * initTokenizer / tokenizerEncode / tokenizerDecode (c_binding.cpp:17-28,122-135) are three forwarding shims to the
//     reference's own GPT2Tokenizer: they exist when the module is built with the reference's include directory on the
//     path (include/rwkv.h pulls in rwkv/tokenizer/tokenizer.h through __has_include); the tokenizer itself is outside
//     this engine's scope and is not re-implemented here.  tokenizerEncode converts vector<long long> -> vector<int64_t>
//     explicitly (the reference's own line c_binding.cpp:126 does not compile on LP64 Linux).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "rwkv.h"
#include "rwkv_sampler.h"

namespace py = pybind11;

static RWKV *M(std::uintptr_t h) { return reinterpret_cast<RWKV *>(h); }

PYBIND11_MODULE(rwkv, m)
{
    m.def("initRwkv", []() { return reinterpret_cast<std::uintptr_t>(new RWKV()); }, "initRwkv");
    m.def("freeRwkv", [](std::uintptr_t h) { delete M(h); }, "destroy a handle (engine extension)");
    m.def("loadModel", [](std::uintptr_t h, const std::string &filename, unsigned long long maxGPT) {
        M(h)->loadFile(filename, maxGPT);
        return std::make_tuple((int64_t)M(h)->num_layers, (int64_t)M(h)->num_embed);
    }, "load (maxGPT: state slots and logits rows, 1 as in the reference; decodeBeam needs its width)", py::arg("rwkvp"), py::arg("filename"), py::arg("maxGPT") = 1ull);
    m.def("modelForward", [](std::uintptr_t h, int64_t token) { M(h)->forward((unsigned long long)token); }, "rwkvc");
    m.def("initState", [](std::uintptr_t h) {
        RWKV *r = M(h);
        const size_t n = r->num_layers * r->num_embed * r->maxContext;
        for (size_t i = 0; i < n; i++)
            r->state->statexy[i] = r->state->stateaa[i] = r->state->statebb[i] = r->state->statepp[i] = r->state->statedd[i] = 0;
        if (r->residentState) r->pushState();
    }, "initState");
    m.def("getState", [](std::uintptr_t h) {
        RWKV *r = M(h);
        if (r->residentState) r->pullState();
        const size_t n = r->num_layers * r->num_embed;
        py::list out;
        double *src[5] = {r->state->statexy, r->state->stateaa, r->state->statebb, r->state->statepp, r->state->statedd};
        for (int s = 0; s < 5; s++) {
            py::array_t<double> a(n);
            std::copy(src[s], src[s] + n, a.mutable_data());
            out.append(a);
        }
        return out;
    }, "getRwkvState");
    m.def("initOutput", [](std::uintptr_t h) { std::fill(M(h)->out, M(h)->out + 50277, 0.f); }, "initOutput");
    m.def("getOutput", [](std::uintptr_t h) {
        py::array_t<float> a(50277);
        std::copy(M(h)->out, M(h)->out + 50277, a.mutable_data());
        return a;
    }, "getRwkvOutput");
    m.def("typicalSample", [](std::uintptr_t h, float temp, float tau) { return typical(M(h)->out, temp, tau); },
          "typicalSample", py::arg("rwkvp"), py::arg("temp") = 0.9f, py::arg("tau") = 0.8f);
#ifdef RWKV_HAVE_TOKENIZER
    m.def("initTokenizer", [](const std::string &vocab_filename, const std::string &merges_filename) {
        std::optional<GPT2Tokenizer> t = GPT2Tokenizer::load(vocab_filename, merges_filename);
        if (!t.has_value()) {
            std::cerr << "Failed to load tokenizer" << std::endl;
            throw py::value_error("Failed to load tokenizer");
        }
        return reinterpret_cast<std::uintptr_t>(new GPT2Tokenizer(t.value()));
    }, "initTokenizer");
    m.def("tokenizerEncode", [](std::uintptr_t tp, std::string s) {
        const auto ids = reinterpret_cast<GPT2Tokenizer *>(tp)->encode(s);
        return std::vector<int64_t>(ids.begin(), ids.end());
    }, "tokenizerEncode");
    m.def("tokenizerDecode", [](std::uintptr_t tp, int token) {
        return reinterpret_cast<GPT2Tokenizer *>(tp)->decode({(long int)token});
    }, "tokenizerDecode");
#endif
    m.def("setResident", [](std::uintptr_t h, bool on) { M(h)->residentState = on; }, "keep state on the device (engine extension)");
    m.def("decodeGreedy", [](std::uintptr_t h, int64_t first, int64_t n) { return M(h)->decodeGreedy(first, n); },
          "device-side greedy continuation (engine extension)");
    m.def("nucleusSample", [](std::uintptr_t h, float temp, float top_p, unsigned top_k, float presence, float frequency, float decay, bool ban0) {
        const double u = std::generate_canonical<double, 53>(rwkv_sampler_rng());
        return M(h)->sampleNucleus(RWKV::Nucleus{temp, top_p, top_k, presence, frequency, decay}, u < 1.0 ? u : 0.0, ban0, true);
    }, "draw the next token ON THE DEVICE from the logits of the last modelForward: temperature, top-p, top-k, presence / frequency penalties on the "
       "context's decaying occurrence counts, which the pick updates (engine extension)",
          py::arg("rwkvp"), py::arg("temp") = 1.0f, py::arg("top_p") = 0.9f, py::arg("top_k") = 0u, py::arg("presence") = 0.f,
          py::arg("frequency") = 0.f, py::arg("decay") = 1.0f, py::arg("ban0") = false);
    m.def("decodeNucleus", [](std::uintptr_t h, int64_t first, int64_t n, float temp, float top_p, unsigned top_k, float presence, float frequency,
                              float decay, uint64_t seed, bool keep) {
        return M(h)->decodeNucleus(first, n, RWKV::Nucleus{temp, top_p, top_k, presence, frequency, decay}, seed, keep);
    }, "device-side continuation with the nucleus sampler (engine extension)",
          py::arg("rwkvp"), py::arg("first"), py::arg("n"), py::arg("temp") = 1.0f, py::arg("top_p") = 0.9f, py::arg("top_k") = 0u,
          py::arg("presence") = 0.f, py::arg("frequency") = 0.f, py::arg("decay") = 1.0f, py::arg("seed") = 0ull, py::arg("keep") = false);
    m.def("decodeUntil", [](std::uintptr_t h, int64_t first, int64_t n, float temp, float top_p, unsigned top_k, float presence, float frequency,
                            float decay, uint64_t seed, bool keep, const std::vector<std::vector<int64_t>> &stops) {
        RWKV::Stop stop;
        for (const auto &q : stops) stop.sequences.emplace_back(q.begin(), q.end());
        stop.keep = keep;
        RWKV::Until r = M(h)->decodeBatchUntil({(unsigned long long)first}, n, RWKV::Pick::nucleus(RWKV::Nucleus{temp, top_p, top_k, presence, frequency, decay}),
                                               {seed}, stop);
        r.ids.resize(r.len[0]);
        return std::make_tuple(std::vector<int64_t>(r.ids.begin(), r.ids.end()), (int)r.reason[0]);
    }, "decodeNucleus that ends at the first of the stop sequences `stops` (lists of token ids): returns (ids up to and including the end of the "
       "match, reason: 0 ran all n, 2 + j matched stops[j]); the state is left where the stream stopped -- feed ids[-1] to go on (engine extension)",
          py::arg("rwkvp"), py::arg("first"), py::arg("n"), py::arg("temp") = 1.0f, py::arg("top_p") = 0.9f, py::arg("top_k") = 0u,
          py::arg("presence") = 0.f, py::arg("frequency") = 0.f, py::arg("decay") = 1.0f, py::arg("seed") = 0ull, py::arg("keep") = false,
          py::arg("stops") = std::vector<std::vector<int64_t>>{});
    m.def("scoreTokens", [](std::uintptr_t h, const std::vector<int64_t> &tokens) {
        const RWKV::Scores s = M(h)->score(std::vector<unsigned long long>(tokens.begin(), tokens.end()));
        py::array_t<double> a(s.logprob.size());
        std::copy(s.logprob.begin(), s.logprob.end(), a.mutable_data());
        return a;
    }, "f64 log-probabilities of tokens[1:], each under the logits that follow its predecessor, computed on the device (engine extension)");
    m.def("topLogprobs", [](std::uintptr_t h, const std::vector<int64_t> &rows, unsigned top_n) {
        const RWKV::TopN t = M(h)->topnRows(std::vector<unsigned long long>(rows.begin(), rows.end()), top_n);
        py::array_t<int64_t> ids({rows.size(), (size_t)top_n});
        py::array_t<double> lp({rows.size(), (size_t)top_n});
        std::copy(t.ids.begin(), t.ids.end(), ids.mutable_data());
        std::copy(t.logprob.begin(), t.logprob.end(), lp.mutable_data());
        return py::make_tuple(ids, lp);
    }, "(ids, f64 log-probabilities) [len(rows)][top_n]: the top_n most probable tokens of logits rows of the last forward, computed on the device (engine extension)");
    m.def("decodeBeam", [](std::uintptr_t h, int64_t first, int64_t n, unsigned width, const std::vector<int64_t> &stops) {
        RWKV::Beam beam;
        beam.width = width;
        beam.stop_ids.assign(stops.begin(), stops.end());
        const RWKV::BeamResult r = M(h)->decodeBeam((unsigned long long)first, (unsigned long long)n, beam);
        py::array_t<int64_t> tokens({(size_t)width, (size_t)n}), len((size_t)width);
        py::array_t<double> score((size_t)width), lp({(size_t)width, (size_t)n});
        std::copy(r.tokens.begin(), r.tokens.end(), tokens.mutable_data());
        std::copy(r.len.begin(), r.len.end(), len.mutable_data());
        std::copy(r.score.begin(), r.score.end(), score.mutable_data());
        std::copy(r.token_logprob.begin(), r.token_logprob.end(), lp.mutable_data());
        return py::make_tuple(tokens, len, score, lp);
    }, "beam search ON THE DEVICE from the state slot 0 holds (load with maxGPT >= width): (tokens [width][n], len [width], score [width], "
       "token log-probs [width][n]); hypothesis 0 is the best, entries behind a hypothesis's end are 0 (engine extension)",
          py::arg("rwkvp"), py::arg("first"), py::arg("n"), py::arg("width") = 4u, py::arg("stops") = std::vector<int64_t>{});
    m.def("specVerify", [](std::uintptr_t h, int64_t token, const std::vector<int64_t> &draft) {
        const RWKV::SpecStep s = M(h)->specVerify((unsigned long long)token, std::vector<unsigned long long>(draft.begin(), draft.end()));
        return py::make_tuple((int64_t)s.accepted, (int64_t)s.next);
    }, "feed [token, *draft] to slot 0 in one pass of the chunk path and keep the longest prefix of the draft the greedy picks confirm: "
       "(n_accepted, next); next is emitted, not fed (engine extension)", py::arg("rwkvp"), py::arg("token"), py::arg("draft") = std::vector<int64_t>{});
    m.def("decodeSpeculative", [](std::uintptr_t h, std::uintptr_t draft, int64_t first, int64_t n, unsigned k) {
        if (n < 1) throw std::runtime_error("n must be at least 1");
        const RWKV::SpecResult r = M(h)->decodeSpeculative(*M(draft), (unsigned long long)first, (unsigned long long)n, k);
        py::array_t<int64_t> ids((size_t)n);
        std::copy(r.tokens.begin(), r.tokens.end(), ids.mutable_data());
        return py::make_tuple(ids, py::make_tuple((int64_t)r.rounds, (int64_t)r.drafted, (int64_t)r.accepted));
    }, "speculative greedy decoding: the model of handle `draft` (loaded with maxGPT >= k + 2, same prefix in slot 0) guesses k ids per round, this "
       "one verifies them in one pass: (ids [n], (rounds, drafted, accepted)); the ids do not depend on the draft model (engine extension)",
          py::arg("rwkvp"), py::arg("draft"), py::arg("first"), py::arg("n"), py::arg("k") = 4u);
    m.def("modelForwardSegments", [](std::uintptr_t h, const std::vector<std::pair<unsigned, std::vector<int64_t>>> &segments) {
        std::vector<RWKV::Segment> segs;
        for (const auto &s : segments) segs.push_back(RWKV::Segment{s.first, std::vector<unsigned long long>(s.second.begin(), s.second.end())});
        const std::vector<unsigned long long> last = M(h)->forwardSegments(segs);
        return std::vector<int64_t>(last.begin(), last.end());
    }, "one call of the chunk path over segments [(slot, ids)] with pairwise distinct slots: every sequence continues from its slot, logits row j "
       "belongs to token j of the ids back to back; returns the row of each segment's last token (engine extension)", py::arg("rwkvp"), py::arg("segments"));
    // ---- constrained decoding: the engine calls, and the host twins of include/rwkv_sampler.h for the suite ----
    using u32arr = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>;
    using f32arr = py::array_t<float, py::array::c_style | py::array::forcecast>;
    m.def("setConstraint", [](std::uintptr_t h, u32arr row_ptr, u32arr tok, u32arr next) {
        RWKV::Automaton a;
        a.row_ptr.assign(row_ptr.data(), row_ptr.data() + row_ptr.size()); a.tok.assign(tok.data(), tok.data() + tok.size());
        a.next.assign(next.data(), next.data() + next.size());
        M(h)->setConstraint(a);
    }, "install a token-level automaton in CSR form (row_ptr [S + 1], tok [nnz], next [nnz]; a state without edges is terminal): every later "
       "decodeConstrained generates only what it allows (engine extension)");
    m.def("clearConstraint", [](std::uintptr_t h) { M(h)->clearConstraint(); }, "remove the installed automaton (engine extension)");
    m.def("decodeConstrained", [](std::uintptr_t h, int64_t first, int64_t n, float temp, float top_p, unsigned top_k, float presence, float frequency,
                                  float decay, uint64_t seed, bool greedy, const std::vector<uint32_t> &bias_tok, const std::vector<float> &bias_val) {
        const RWKV::Pick pick = greedy ? RWKV::Pick::greedy() : RWKV::Pick::nucleus(RWKV::Nucleus{temp, top_p, top_k, presence, frequency, decay});
        std::vector<RWKV::Bias> bias;
        if (!bias_tok.empty()) bias.push_back(RWKV::Bias{bias_tok, bias_val});
        RWKV::Constrained r = M(h)->decodeConstrained({(unsigned long long)first}, n, pick, {seed}, RWKV::Stop{}, {0u}, bias);
        r.until.ids.resize(r.until.len[0]);
        return std::make_tuple(std::vector<int64_t>(r.until.ids.begin(), r.until.ids.end()), (int)r.until.reason[0], (int)r.state[0]);
    }, "device-side continuation under the installed automaton from its state 0, with an optional logit bias (ids ascending; -inf bans): returns "
       "(ids, reason: 0 ran all n, 32 the automaton reached a terminal state, automaton state) (engine extension)",
          py::arg("rwkvp"), py::arg("first"), py::arg("n"), py::arg("temp") = 1.0f, py::arg("top_p") = 0.9f, py::arg("top_k") = 0u,
          py::arg("presence") = 0.f, py::arg("frequency") = 0.f, py::arg("decay") = 1.0f, py::arg("seed") = 0ull, py::arg("greedy") = false,
          py::arg("bias_tok") = std::vector<uint32_t>{}, py::arg("bias_val") = std::vector<float>{});
    m.def("constraintCheck", [](py::object S, py::object row_ptr, py::object tok, py::object next, py::object bias_tok, py::object bias_val) -> py::object {
        // the arrays as given: S and the lengths are NOT derived from each other, so that every malformed input reaches the validator
        u32arr rp, tk, nx, bt;
        f32arr bv;
        constraint_view a{};
        bias_view b{};
        const bool has_a = !S.is_none(), has_b = !bias_tok.is_none();
        if (has_a) {
            rp = row_ptr.cast<u32arr>(); tk = tok.cast<u32arr>(); nx = next.cast<u32arr>();
            const unsigned long long s = S.cast<unsigned long long>();
            if ((unsigned long long)rp.size() != s + 1 && !(s == 0 || s > 4096ull)) throw py::value_error("constraintCheck: row_ptr has S + 1 entries");
            if (tk.size() != nx.size()) throw py::value_error("constraintCheck: tok and next have nnz entries");
            a = constraint_view{s, rp.data(), (unsigned long long)tk.size(), tk.data(), nx.data()};
        }
        if (has_b) {
            bt = bias_tok.cast<u32arr>(); bv = bias_val.cast<f32arr>();
            if (bt.size() != bv.size()) throw py::value_error("constraintCheck: one value per bias id");
            b = bias_view{(unsigned long long)bt.size(), bt.data(), bv.data()};
        }
        const char *rule = constraint_check(has_a ? &a : nullptr, has_b ? &b : nullptr);
        return rule ? py::object(py::str(rule)) : py::object(py::none());
    }, "the ONE validator of automata and bias lists ON THE HOST (include/rwkv_sampler.h constraint_check): None when well formed, else the name "
       "of the first rule broken (engine extension)",
          py::arg("S") = py::none(), py::arg("row_ptr") = py::none(), py::arg("tok") = py::none(), py::arg("next") = py::none(),
          py::arg("bias_tok") = py::none(), py::arg("bias_val") = py::none());
    m.def("constrainedRow", [](f32arr logits, py::object row_ptr, py::object tok, py::object next, unsigned q, py::object bias_tok, py::object bias_val) {
        if (logits.size() != 50277) throw py::value_error("constrainedRow: 50277 logits");
        u32arr rp, tk, nx, bt;
        f32arr bv;
        constraint_view a{};
        bias_view b{};
        if (!row_ptr.is_none()) {
            rp = row_ptr.cast<u32arr>(); tk = tok.cast<u32arr>(); nx = next.cast<u32arr>();
            a = constraint_view{(unsigned long long)rp.size() - 1, rp.data(), (unsigned long long)tk.size(), tk.data(), nx.data()};
            if (constraint_check(&a, nullptr) || q >= a.S) throw py::value_error("constrainedRow: malformed automaton or state");
        }
        if (!bias_tok.is_none()) {
            bt = bias_tok.cast<u32arr>(); bv = bias_val.cast<f32arr>();
            b = bias_view{(unsigned long long)bt.size(), bt.data(), bv.data()};
            if (bt.size() != bv.size() || constraint_check(nullptr, &b)) throw py::value_error("constrainedRow: malformed bias list");
        }
        py::array_t<float> c(50277);
        constrained_row(logits.data(), row_ptr.is_none() ? nullptr : &a, q, bias_tok.is_none() ? nullptr : &b, c.mutable_data());
        return c;
    }, "the constrained row ON THE HOST (include/rwkv_sampler.h constrained_row, the twin of the device's): f32 [50277] (engine extension)",
          py::arg("logits"), py::arg("row_ptr") = py::none(), py::arg("tok") = py::none(), py::arg("next") = py::none(), py::arg("q") = 0u,
          py::arg("bias_tok") = py::none(), py::arg("bias_val") = py::none());
    m.def("constraintNext", [](u32arr row_ptr, u32arr tok, u32arr next, unsigned q, unsigned g) {
        const constraint_view a{(unsigned long long)row_ptr.size() - 1, row_ptr.data(), (unsigned long long)tok.size(), tok.data(), next.data()};
        if (constraint_check(&a, nullptr) || q >= a.S) throw py::value_error("constraintNext: malformed automaton or state");
        return constraint_next(&a, q, g);
    }, "the automaton state after pick g in state q ON THE HOST (include/rwkv_sampler.h constraint_next) (engine extension)");
    m.def("constraintTrie", [](const std::vector<std::vector<unsigned long long>> &choices) {
        const constraint_automaton A = constraint_trie(choices);
        return py::make_tuple(py::array_t<uint32_t>(A.row_ptr.size(), A.row_ptr.data()), py::array_t<uint32_t>(A.tok.size(), A.tok.data()),
                              py::array_t<uint32_t>(A.next.size(), A.next.data()));
    }, "(row_ptr, tok, next) of the automaton that spells exactly one of the given token sequences (include/rwkv_sampler.h constraint_trie) (engine extension)");
    m.def("beamSelect", [](py::array_t<int64_t, py::array::c_style | py::array::forcecast> top_ids, py::array_t<double, py::array::c_style | py::array::forcecast> top_lp,
                           py::array_t<double, py::array::c_style | py::array::forcecast> cum, const std::vector<int> &ended, const std::vector<int64_t> &last,
                           const std::vector<int64_t> &stops) {
        const size_t W = (size_t)cum.size();
        if (W < 1 || (size_t)top_ids.size() != W * (W + 1) || (size_t)top_lp.size() != W * (W + 1) || ended.size() != W || last.size() != W)
            throw py::value_error("beamSelect: top_ids and top_lp [W][W + 1], cum, ended and last [W]");
        std::vector<unsigned long long> ids(top_ids.data(), top_ids.data() + W * (W + 1)), l(last.begin(), last.end()), st(stops.begin(), stops.end());
        std::vector<unsigned char> e(ended.begin(), ended.end());
        const std::vector<beam_pick> r = beam_select((unsigned)W, ids.data(), top_lp.data(), cum.data(), e.data(), l.data(), st);
        py::array_t<int64_t> parent(r.size()), token(r.size()), end(r.size());
        py::array_t<double> score(r.size()), lp(r.size());
        for (size_t m = 0; m < r.size(); m++) {
            parent.mutable_data()[m] = r[m].parent; token.mutable_data()[m] = (int64_t)r[m].token; end.mutable_data()[m] = r[m].ended ? 1 : 0;
            score.mutable_data()[m] = r[m].score; lp.mutable_data()[m] = r[m].token_logprob;
        }
        return py::make_tuple(parent, token, score, lp, end);
    }, "one beam-search selection ON THE HOST (include/rwkv_sampler.h beam_select, the twin of the device's): from the rows' top W + 1 ids and "
       "log-probs, cum, ended and last [W] and the stop ids -> (parent, token, score, token log-prob, ended) [W] (engine extension)");
}
