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
