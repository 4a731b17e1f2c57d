// rwkv.h -- C++ drop-in for the reference's host API (reference include/rwkv.h ->
// include/rwkv/rwkv/rwkv.h: enum MODE, class RWKVState :140-242, class RWKV :245-429),
// re-implemented as a thin header-only wrapper over the C-ABI of librwkv_mi355x.so
// (include/rwkv_mi355x.h).  Same public names, argument meaning and error behaviour, so the
// reference's callers (examples/*/*.cpp, bindings/pybind/c_binding.cpp) compile against it:
//
//     g++ -std=c++17 app.cpp -I<repo>/include -L<repo>/rwkv-cpp-accelerated_amd/csrc -lrwkv_mi355x
//
// Differences, all documented in INTEGRATION.md:
//   * `tensors[i]` holds the device pointer of slot i where the engine keeps that tensor in file layout (the f32/f64
//     vectors, the five state arrays, X, BUFFER2 = logits; rwkv_tensor_device) and NULL for the uint8 matrices, which
//     are re-tiled at load, and for pure scratch; getTensorSize()/getTensorTypes() answer from the format table.
//   * `residentState = true` keeps the state on the device between calls (the reference re-uploads
//     and re-downloads 5 x L x D doubles around every forward, rwkv.h:353,372); the default keeps
//     the reference's host-authoritative semantics.
//   * like the reference's umbrella include/rwkv.h:1-3 this header also brings in the sampler (`typical`,
//     include/rwkv_sampler.h) and the tokenizer.  The tokenizer (GPT-NeoX BPE) is outside this engine's
//     scope and is NOT re-implemented: when the reference's own include/rwkv/tokenizer/tokenizer.h is on
//     the include path (-I<reference>/include) it is pulled in as it is and `RWKV::loadTokenizer` /
//     `loadContext(std::string)` (rwkv.h:312-319,395-413) forward to it; without it those two members do
//     not exist and loadContext() takes token ids.  Define RWKV_NO_TOKENIZER to keep it out.
//   * decodeGreedy()/decodeTypical() run on the device state.  In the default host-authoritative mode they
//     upload `state` first and download it afterwards, so a following forward() continues the sequence.
#ifndef RWKV_H
#define RWKV_H

#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "rwkv_mi355x.h"
#include "rwkv_sampler.h"
#if !defined(RWKV_NO_TOKENIZER) && !defined(RWKV_HAVE_TOKENIZER) && defined(__has_include)
#if __has_include("rwkv/tokenizer/tokenizer.h")
#include "rwkv/tokenizer/tokenizer.h"   // the reference's GPT2Tokenizer, compiled from where it lies
#define RWKV_HAVE_TOKENIZER 1
#endif
#endif

enum MODE { PARRALEL, GPT };   // reference enums/enum.h:2-5

// tensor-slot indices of model.bin, reference enums/enum.h:7-55
enum {
    X, EMBED, LAYERNORMS, STATEXY, STATEAA, STATEBB, STATEPP, STATEDD, BUFFER1, BUFFER2, BUFFER3, BUFFER4,
    MIXK, MIXV, MIXR, KM, VM, RM, KR, VR, RR, O1, O2, O3, ATTOUT, ATTOUTR, ATTOUTO, FFNMIXK, FFNMIXV,
    FFNK, FFNV, FFNR, FFNKR, FFNVR, FFNRR, FFNKO, FFNVO, FFNRO, FFNKBUFFER, FFNVBUFFER, FFNRBUFFER,
    DECAY, BONUS, HEAD, HEADR, HEADO
};

namespace rwkv_detail {
inline unsigned long long tensor_size(unsigned long long i, unsigned long long a, unsigned long long b)
{   // reference rwkv.h:124-128
    const unsigned long long V = RWKV_VOCAB;
    const unsigned long long s[46] = {b, V * b, 4 * (a + 1) * b, a * b, a * b, a * b, a * b, a * b, b, V, b, b,
        a * b, a * b, a * b, a * b * b, a * b * b, a * b * b, a * b, a * b, a * b, a * b, a * b, a * b,
        a * b * b, a * b, a * b, a * b, a * b, a * b * b * 4, a * b * b * 4, a * b * b,
        a * b, a * b * 4, a * b, a * b, a * b * 4, a * b, b, b, b * 4, a * b, a * b, V * b, b, b};
    return s[i];
}
inline unsigned long long tensor_type(unsigned long long i)
{   // reference rwkv.h:84
    const unsigned long long t[46] = {8, 4, 8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 8, 8, 8, 1, 1, 1, 4, 4, 4, 4, 4,
                                      4, 1, 4, 4, 8, 8, 1, 1, 1, 4, 4, 4, 4, 4, 4, 8, 8, 4, 8, 8, 1, 4, 4};
    return t[i];
}
inline void check(int rc)
{
    if (rc != RWKV_OK) throw std::runtime_error(rwkv_last_error());
}
} // namespace rwkv_detail

// reference rwkv.h:140-242 -- five host arrays [stateSize][num_layers][num_embed] doubles, value type
class RWKVState
{
public:
    double *statexy, *stateaa, *statebb, *statepp, *statedd;
    unsigned long long num_layers, num_embed, stateSize;

    RWKVState(unsigned long long num_layers, unsigned long long num_embed, unsigned long long stateSize)
        : num_layers(num_layers), num_embed(num_embed), stateSize(stateSize)
    {
        alloc();
        for (unsigned long long i = 0; i < total(); i++) statexy[i] = stateaa[i] = statebb[i] = statepp[i] = statedd[i] = 0;
    }
    RWKVState(const RWKVState &o) : num_layers(o.num_layers), num_embed(o.num_embed), stateSize(o.stateSize)
    {
        alloc();
        copy_from(o, 0, 0, total());
    }
    // sub-state `offset` of `o` as a 1-slot state (the reference ignores the L*D stride here,
    // rwkv.h:205-209 -- only offset 0 is ever used by its callers; this one honours it)
    RWKVState(const RWKVState &o, unsigned long long offset) : num_layers(o.num_layers), num_embed(o.num_embed), stateSize(1)
    {
        alloc();
        copy_from(o, offset * num_layers * num_embed, 0, num_layers * num_embed);
    }
    RWKVState &operator=(const RWKVState &o)
    {
        if (this != &o) {
            release();
            num_layers = o.num_layers; num_embed = o.num_embed; stateSize = o.stateSize;
            alloc();
            copy_from(o, 0, 0, total());
        }
        return *this;
    }
    ~RWKVState() { release(); }

    RWKVState getSubState(unsigned long long offset = 0)
    {
        if (offset >= stateSize)
            throw std::runtime_error("State get offset out of bounds, max offset is " + std::to_string(stateSize));
        return RWKVState(*this, offset);
    }
    void setSubState(RWKVState &other, unsigned long long offset = 0)
    {
        const unsigned long long n = num_layers * num_embed;
        for (unsigned long long i = 0; i < n; i++) {
            statexy[i + offset * n] = other.statexy[i]; stateaa[i + offset * n] = other.stateaa[i];
            statebb[i + offset * n] = other.statebb[i]; statepp[i + offset * n] = other.statepp[i];
            statedd[i + offset * n] = other.statedd[i];
        }
    }

private:
    unsigned long long total() const { return num_layers * num_embed * stateSize; }
    void alloc()
    {
        const unsigned long long n = total();
        statexy = new double[n]; stateaa = new double[n]; statebb = new double[n]; statepp = new double[n]; statedd = new double[n];
    }
    void release() { delete[] statexy; delete[] stateaa; delete[] statebb; delete[] statepp; delete[] statedd; }
    void copy_from(const RWKVState &o, unsigned long long src, unsigned long long dst, unsigned long long n)
    {
        for (unsigned long long i = 0; i < n; i++) {
            statexy[dst + i] = o.statexy[src + i]; stateaa[dst + i] = o.stateaa[src + i]; statebb[dst + i] = o.statebb[src + i];
            statepp[dst + i] = o.statepp[src + i]; statedd[dst + i] = o.statedd[src + i];
        }
    }
};

class GPT2Tokenizer;   // the reference's tokenizer (see header comment); only ever used through a pointer here

// reference rwkv.h:245-429
class RWKV
{
public:
    int **tensors = new int *[46]();    // reference rwkv.h:248; filled by loadFile (see header comment)
    unsigned long long num_layers = 0;
    unsigned long long num_embed = 0;
    float *out = nullptr;               // host logits [maxContext][50277]; forward() returns this
    unsigned long long maxContext = 1;
    RWKVState *state = nullptr;         // host state (authoritative unless residentState)
    GPT2Tokenizer *tokenizer = nullptr;
    bool ready = false;
    bool residentState = false;         // engine extension: keep state on the device between forwards
    // deprecated aliases of state->*, reference rwkv.h:270-274
    double *statexy = nullptr, *stateaa = nullptr, *statebb = nullptr, *statepp = nullptr, *statedd = nullptr;

    RWKV() {}
    explicit RWKV(int device) : device_(device) {}
    RWKV(const RWKV &) = delete;
    RWKV &operator=(const RWKV &) = delete;

    void loadFile(const std::string &filename, unsigned long long maxGPT = 1)
    {
        if (ready) throw std::runtime_error("RWKV already loaded");
        ensure_ctx();
        const int rc = rwkv_load_file(ctx_, filename.c_str(), maxGPT);
        if (rc == RWKV_E_IO) {   // the reference prints and exit(1)s (rwkv.cu:641-645); a library throws instead
            std::cout << rwkv_last_error() << std::endl;
            throw std::runtime_error(rwkv_last_error());
        }
        rwkv_detail::check(rc);
        num_layers = rwkv_n_layers(ctx_);
        num_embed = rwkv_n_embed(ctx_);
        for (int i = 0; i < 46; i++) tensors[i] = static_cast<int *>(rwkv_tensor_device(ctx_, i));
        std::cout << "n_layers: " << num_layers << std::endl << "n_embed: " << num_embed << std::endl;   // rwkv.cu:653-654
        state = new RWKVState(num_layers, num_embed, maxGPT);
        statexy = state->statexy; stateaa = state->stateaa; statebb = state->statebb; statepp = state->statepp; statedd = state->statedd;
        out = new float[(size_t)RWKV_VOCAB * maxGPT]();
        maxContext = maxGPT;
        ready = true;
    }

    unsigned long long getTensorSize(unsigned long long i) { return rwkv_detail::tensor_size(i, num_layers, num_embed); }
    unsigned long long getTensorTypes(unsigned long long i) { return rwkv_detail::tensor_type(i); }

    float *forward(std::vector<unsigned long long> token, MODE mode)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (token.size() > maxContext)
            throw std::runtime_error("Context too large, max context is " + std::to_string(maxContext));
        const uint64_t T = token.size();
        std::vector<uint64_t> t64(token.begin(), token.end());
        if (!residentState)   // setState, rwkv.h:353
            rwkv_detail::check(rwkv_set_state(ctx_, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, T));
        rwkv_detail::check(rwkv_forward(ctx_, t64.data(), T, mode == PARRALEL ? RWKV_MODE_PARRALEL : RWKV_MODE_GPT));
        if (residentState)
            rwkv_detail::check(rwkv_get_output(ctx_, out, nullptr, nullptr, nullptr, nullptr, nullptr, T));
        else                  // getOutput, rwkv.h:372
            rwkv_detail::check(rwkv_get_output(ctx_, out, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, T));
        return out;
    }
    float *forward(unsigned long long token) { return forward(std::vector<unsigned long long>{token}, GPT); }
    float *forward(std::vector<long long> token, MODE mode)
    {
        std::vector<unsigned long long> t2(token.begin(), token.end());
        return forward(t2, mode);
    }

    RWKVState emptyState() { return RWKVState(num_layers, num_embed, 1); }

    // prompt ingestion in chunks of maxContext tokens, GPT mode (reference rwkv.h:395-413);
    // returns the last prompt token like the reference does
    long long loadContext(const std::vector<long long> &initial, bool progress = false)
    {
        if (initial.empty()) throw std::runtime_error("empty context");
        for (size_t i = 0; i < initial.size(); i += maxContext) {
            const size_t e = std::min(i + (size_t)maxContext, initial.size());
            forward(std::vector<unsigned long long>(initial.begin() + i, initial.begin() + e), GPT);
            if (progress) { std::cout << "\r" << int(float(i) / initial.size() * 100) << "%"; std::flush(std::cout); }
        }
        return initial.back();
    }
#ifdef RWKV_HAVE_TOKENIZER
    // reference rwkv.h:312-319
    void loadTokenizer(std::string vocabPath)
    {
        auto _tokenizer = GPT2Tokenizer::load(vocabPath + "/vocab.json", vocabPath + "/merges.txt");
        if (!_tokenizer.has_value()) {
            std::cerr << "Failed to load tokenizer" << std::endl;
            return;
        }
        tokenizer = new GPT2Tokenizer(_tokenizer.value());
    }
    // reference rwkv.h:395-413 (prints "<first id>:token" like the reference does)
    long long loadContext(std::string input, bool progress = false)
    {
        if (!tokenizer) throw std::runtime_error("tokenizer not loaded");
        const std::vector<long long> initial = widen(tokenizer->encode(input));
        if (!initial.empty()) std::cout << initial[0] << ":token";
        return loadContext(initial, progress);
    }
#endif

    // engine extensions -------------------------------------------------------------------
    // explicit sync points for residentState mode
    void pushState() { rwkv_detail::check(rwkv_set_state(ctx_, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, maxContext)); }
    void pullState() { rwkv_detail::check(rwkv_get_output(ctx_, nullptr, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, maxContext)); }
    // device-side greedy continuation (storygen's loop with argmax; token 0 banned as out[0] = -99 does)
    std::vector<unsigned long long> decodeGreedy(unsigned long long first, unsigned long long n)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        std::vector<uint64_t> ids(n);
        if (!residentState) pushState();      // host state is authoritative: continue from it ...
        rwkv_detail::check(rwkv_decode_greedy(ctx_, first, n, ids.data()));
        if (!residentState) pullState();      // ... and leave it where the generated tokens ended
        return std::vector<unsigned long long>(ids.begin(), ids.end());
    }
    // typical sampling on the device from the logits of the last forward (no 201 KB download, no host sort);
    // u in [0, 1) is the caller's uniform, the draw is the inverse CDF in token order (rwkv_sampler.h typical_u)
    int sampleTypical(float temp, float tau, double u, bool ban0 = false, unsigned long long row = 0, bool recipe = RWKV_TYPICAL_RECIPE != 0)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        uint64_t tok = 0;
        rwkv_detail::check(rwkv_sample_typical(ctx_, row, temp, tau, u, (ban0 ? RWKV_SAMPLE_BAN0 : 0) | (recipe ? RWKV_SAMPLE_RECIPE : 0), &tok));
        return (int)tok;
    }
    // device-side sampled continuation: storygen's loop (examples/storygen/storygen.cpp:63-69) without host round trips
    std::vector<unsigned long long> decodeTypical(unsigned long long first, unsigned long long n, float temp = 0.9f, float tau = 0.8f,
                                                  unsigned long long seed = 0, bool recipe = RWKV_TYPICAL_RECIPE != 0)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        std::vector<uint64_t> ids(n);
        if (!residentState) pushState();
        rwkv_detail::check(rwkv_decode_typical(ctx_, first, n, temp, tau, seed, recipe ? RWKV_SAMPLE_RECIPE : 0, ids.data()));
        if (!residentState) pullState();
        return std::vector<unsigned long long>(ids.begin(), ids.end());
    }
    // batched decode: first.size() independent streams, stream s on state slot s; ids[s * n + k] = stream s's pick at step k.
    // In the host-authoritative mode the N slots are pushed before the call and pulled after it, as decodeGreedy does for slot 0.
    std::vector<unsigned long long> decodeBatchGreedy(const std::vector<unsigned long long> &first, unsigned long long n)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        std::vector<uint64_t> ft(first.begin(), first.end()), ids(first.size() * n);
        if (!residentState) pushState();
        rwkv_detail::check(rwkv_decode_batch_greedy(ctx_, ft.data(), ft.size(), n, ids.data()));
        if (!residentState) pullState();
        return std::vector<unsigned long long>(ids.begin(), ids.end());
    }
    // the same with the device sampler: stream s draws what decodeTypical(first[s], n, temp, tau, seeds[s]) draws
    std::vector<unsigned long long> decodeBatchTypical(const std::vector<unsigned long long> &first, unsigned long long n,
                                                       const std::vector<unsigned long long> &seeds, float temp = 0.9f, float tau = 0.8f,
                                                       bool recipe = RWKV_TYPICAL_RECIPE != 0)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (seeds.size() != first.size()) throw std::runtime_error("need one seed per stream");
        std::vector<uint64_t> ft(first.begin(), first.end()), sd(seeds.begin(), seeds.end()), ids(first.size() * n);
        if (!residentState) pushState();
        rwkv_detail::check(rwkv_decode_batch_typical(ctx_, ft.data(), ft.size(), n, temp, tau, sd.data(), recipe ? RWKV_SAMPLE_RECIPE : 0, ids.data()));
        if (!residentState) pullState();
        return std::vector<unsigned long long>(ids.begin(), ids.end());
    }
    // nucleus sampling with repetition penalties on the device (rwkv_mi355x.h "nucleus sampling"): temperature, top-p, top-k, presence and
    // frequency penalties on the occurrence counts the context keeps per state slot.  The plain values of one call:
    struct Nucleus { float temp = 1.0f, top_p = 0.9f; unsigned top_k = 0; float presence = 0.f, frequency = 0.f, decay = 1.0f; };
    static rwkv_nucleus_params nucleusParams(const Nucleus &s, unsigned flags) { return rwkv_nucleus_params{s.temp, s.top_p, s.top_k, s.presence, s.frequency, s.decay, flags, 0u}; }
    // one draw from logits row `row` of the last forward with the counts of slot `slot`; update: count the pick (counts * decay, then + 1)
    int sampleNucleus(const Nucleus &s, double u, bool ban0 = false, bool update = false, unsigned long long row = 0, unsigned long long slot = 0)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        uint64_t tok = 0;
        const rwkv_nucleus_params p = nucleusParams(s, (ban0 ? RWKV_NUCLEUS_BAN0 : 0u) | (update ? RWKV_NUCLEUS_UPDATE : 0u));
        rwkv_detail::check(rwkv_sample_nucleus(ctx_, row, slot, &p, u, &tok));
        return (int)tok;
    }
    // device-side sampled continuation on slot 0 (logit 0 banned, counts updated every step); keep: go on from the counts the last call left
    std::vector<unsigned long long> decodeNucleus(unsigned long long first, unsigned long long n, const Nucleus &s, unsigned long long seed = 0, bool keep = false)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        std::vector<uint64_t> ids(n);
        const rwkv_nucleus_params p = nucleusParams(s, keep ? RWKV_NUCLEUS_KEEP : 0u);
        if (!residentState) pushState();
        rwkv_detail::check(rwkv_decode_nucleus(ctx_, first, n, &p, seed, ids.data()));
        if (!residentState) pullState();
        return std::vector<unsigned long long>(ids.begin(), ids.end());
    }
    // the same for first.size() streams: stream s on slot s draws what decodeNucleus(first[s], n, s, seeds[s]) draws
    std::vector<unsigned long long> decodeBatchNucleus(const std::vector<unsigned long long> &first, unsigned long long n,
                                                       const std::vector<unsigned long long> &seeds, const Nucleus &s, bool keep = false)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (seeds.size() != first.size()) throw std::runtime_error("need one seed per stream");
        std::vector<uint64_t> ft(first.begin(), first.end()), sd(seeds.begin(), seeds.end()), ids(first.size() * n);
        const rwkv_nucleus_params p = nucleusParams(s, keep ? RWKV_NUCLEUS_KEEP : 0u);
        if (!residentState) pushState();
        rwkv_detail::check(rwkv_decode_batch_nucleus(ctx_, ft.data(), ft.size(), n, &p, sd.data(), ids.data()));
        if (!residentState) pullState();
        return std::vector<unsigned long long>(ids.begin(), ids.end());
    }
    // stop sequences and per-stream budgets in the device loops (rwkv_mi355x.h "stop sequences"): stream s ends at the first of `sequences`
    // (token ids, each 1 .. 8 long) that its newest ids spell, or after max_new[s] tokens (empty: no budgets); keep: the match history and --
    // for a nucleus pick with penalties -- the counts go on from the previous call.  Every slot is left as it was when its stream stopped:
    // continue a stream by feeding ids[s * n + len[s] - 1].
    struct Stop { std::vector<std::vector<unsigned long long>> sequences; std::vector<unsigned> max_new; bool keep = false; };
    // how a step picks: Pick::greedy(), Pick::typical(temp, tau, recipe) or Pick::nucleus(s), as the three decodeBatch* calls do
    struct Pick {
        int kind = RWKV_PICK_GREEDY; float temp = 0.9f, tau = 0.8f; bool recipe = false; Nucleus s{};
        static Pick greedy() { return Pick{}; }
        static Pick typical(float temp = 0.9f, float tau = 0.8f, bool recipe = RWKV_TYPICAL_RECIPE != 0) { Pick p; p.kind = RWKV_PICK_TYPICAL; p.temp = temp; p.tau = tau; p.recipe = recipe; return p; }
        static Pick nucleus(const Nucleus &s) { Pick p; p.kind = RWKV_PICK_NUCLEUS; p.s = s; return p; }
    };
    // ids[s * n + k] (0 behind a stream's end), len[s] tokens of stream s count, reason[s]: 0 ran all n, 1 budget, 2 + j sequence j;
    // steps_run: the steps the device was given (rwkv_mi355x.h "bounded run-ahead")
    struct Until { std::vector<unsigned long long> ids; std::vector<unsigned> len, reason; unsigned long long steps_run = 0; };
    Until decodeBatchUntil(const std::vector<unsigned long long> &first, unsigned long long n, const Pick &pick,
                           const std::vector<unsigned long long> &seeds, const Stop &stop)
    {
        return until_call(first, n, pick, seeds, stop, nullptr);
    }
    // log-probs and top-n alternatives of the generated tokens (rwkv_mi355x.h "log-probs and top-n"): decodeBatchUntil that also returns, per
    // stream and step, the log-prob of the pick under the MODEL's distribution (no penalty, no temperature, nothing banned), that row's entropy
    // (entropy = false: left empty) and its top_n most probable ids with their log-probs; 0 / 0.0 behind a stream's end.  Shapes: logprob and
    // entropy [s * n + k], top_ids and top_logprob [(s * n + k) * top_n + j].  Best-of-n ranks forks by the sum of logprob over a stream's len.
    struct Logprobs { Until until; std::vector<double> logprob, entropy; std::vector<unsigned long long> top_ids; std::vector<double> top_logprob; unsigned top_n = 0; };
    Logprobs decodeBatchLogprobs(const std::vector<unsigned long long> &first, unsigned long long n, const Pick &pick,
                                 const std::vector<unsigned long long> &seeds, const Stop &stop, unsigned top_n, bool entropy = true)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (top_n > RWKV_MAX_TOPN) throw std::runtime_error("top_n above RWKV_MAX_TOPN");
        Logprobs r;
        const size_t e = first.size() * n;
        r.top_n = top_n;
        r.logprob.resize(e);
        if (entropy) r.entropy.resize(e);
        std::vector<uint64_t> tid(e * top_n);
        r.top_logprob.resize(e * top_n);
        const rwkv_logprob_out lp{top_n, 0u, r.logprob.data(), entropy ? r.entropy.data() : nullptr, top_n ? tid.data() : nullptr,
                                  top_n ? r.top_logprob.data() : nullptr};
        r.until = until_call(first, n, pick, seeds, stop, &lp);
        r.top_ids.assign(tid.begin(), tid.end());
        return r;
    }
    // the top_n most probable ids of logits rows of the last forward, with their log-probs: ids and logprob [i * top_n + j]; logits and state stay
    struct TopN { std::vector<unsigned long long> ids; std::vector<double> logprob; };
    TopN topnRows(const std::vector<unsigned long long> &rows, unsigned top_n)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        std::vector<uint64_t> r(rows.begin(), rows.end()), ids(rows.size() * top_n);
        TopN t;
        t.logprob.resize(rows.size() * top_n);
        rwkv_detail::check(rwkv_topn_rows(ctx_, r.data(), r.size(), top_n, ids.data(), t.logprob.data()));
        t.ids.assign(ids.begin(), ids.end());
        return t;
    }
    // beam search on the device (rwkv_mi355x.h "beam search"): the `width` most probable continuations of the prompt whose state slot 0 holds,
    // fed `first`, n steps long; stop_ids: single-token stop ids that end a hypothesis.  tokens and token_logprob [m * n + k] (0 / 0.0 from
    // len[m] on), len [m], score [m] = the sum of the token log-probs; hypothesis 0 is the best.  Slot m is left where live hypothesis m ended:
    // feed tokens[m * n + len[m] - 1] to go on.  A length penalty is the caller's: rank by score[m] / pow(len[m], a).
    struct Beam { unsigned width = 4; std::vector<unsigned long long> stop_ids; };
    struct BeamResult { std::vector<unsigned long long> tokens; std::vector<unsigned> len; std::vector<double> score, token_logprob; };
    BeamResult decodeBeam(unsigned long long first, unsigned long long n, const Beam &beam)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (beam.width < 2 || beam.width > RWKV_MAX_BEAM) throw std::runtime_error("beam width outside 2 .. RWKV_MAX_BEAM");
        BeamResult r;
        const size_t W = beam.width;
        std::vector<uint64_t> tok(W * n), stops(beam.stop_ids.begin(), beam.stop_ids.end());
        std::vector<uint32_t> len(W);
        r.score.resize(W); r.token_logprob.resize(W * n);
        const rwkv_beam_params bp{beam.width, (uint32_t)stops.size(), stops.empty() ? nullptr : stops.data(), 0};
        const rwkv_beam_out bo{tok.data(), len.data(), r.score.data(), r.token_logprob.data()};
        if (!residentState) pushState();      // host state is authoritative: the prompt's state is its slot 0 ...
        rwkv_detail::check(rwkv_decode_beam(ctx_, first, n, &bp, &bo));
        if (!residentState) pullState();      // ... and every slot is left where its hypothesis ended
        r.tokens.assign(tok.begin(), tok.end()); r.len.assign(len.begin(), len.end());
        return r;
    }
    // slot m <- what slot parents[m] held, for every m < parents.size() at once (any map: swaps, cycles, fan-out); the other slots stay.
    // Re-fork the survivors of a best-of-n: permuteState({best, best, second, second}).  The host copy too when it is the authoritative one
    void permuteState(const std::vector<unsigned> &parents)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        std::vector<uint32_t> p(parents.begin(), parents.end());
        for (uint32_t v : p) if (v >= p.size()) throw std::runtime_error("a parent outside the map");
        if (!residentState) {
            std::vector<RWKVState> old;
            for (uint32_t v : p) old.push_back(state->getSubState(v));
            for (size_t m = 0; m < p.size(); m++) state->setSubState(old[m], m);
        }
        rwkv_detail::check(rwkv_state_permute(ctx_, p.data(), p.size()));
    }
    // speculative greedy decoding (rwkv_mi355x.h "speculative greedy decoding").  specVerify feeds [token, draft ...] to slot 0 in ONE pass of the
    // chunk path and keeps the longest prefix of the draft that the greedy picks confirm: slot 0 is left behind token, draft[0 .. accepted), and
    // `next` is emitted, not fed.  decodeSpeculative is the loop around it with a draft MODEL (loaded with maxGPT >= k + 2, its slot 0 holding the
    // same prefix): n ids that do not depend on the draft model, both models left behind first, ids[0 .. n - 1).  The verifier is the chunk path:
    // the ids equal decodeGreedy's wherever the top two logits lie further apart than the two paths differ.  In the host-authoritative mode slot 0
    // is pushed before and pulled after, of both models.
    struct SpecStep { unsigned long long accepted, next; };
    struct SpecResult { std::vector<unsigned long long> tokens; unsigned long long rounds, drafted, accepted; };
    SpecStep specVerify(unsigned long long token, const std::vector<unsigned long long> &draft)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        const std::vector<uint64_t> d(draft.begin(), draft.end());
        uint64_t a = 0, nx = 0;
        push_slot0();
        rwkv_detail::check(rwkv_spec_verify(ctx_, token, d.empty() ? nullptr : d.data(), d.size(), &a, &nx));
        pull_slot0();
        return SpecStep{a, nx};
    }
    SpecResult decodeSpeculative(RWKV &draft_model, unsigned long long first, unsigned long long n, unsigned k = 4)
    {
        if (!ready || !draft_model.ready) throw std::runtime_error("RWKV not loaded");
        std::vector<uint64_t> ids(n);
        rwkv_spec_stats st{0, 0, 0};
        push_slot0(); draft_model.push_slot0();
        rwkv_detail::check(rwkv_decode_speculative(ctx_, draft_model.ctx_, first, n, k, ids.data(), &st));
        pull_slot0(); draft_model.pull_slot0();
        return SpecResult{std::vector<unsigned long long>(ids.begin(), ids.end()), st.rounds, st.drafted, st.accepted};
    }
    // segmented forward (rwkv_mi355x.h "segmented forward"): each segment is a run of consecutive tokens of the sequence on state slot `slot`
    // (the slots of one call pairwise distinct); every sequence continues from its slot and leaves it after its tokens, all behind one read of the
    // weights per pass -- decoding streams and pieces of new prompts in one call.  Row j of the logits buffer belongs to token j of the segments'
    // tokens back to back; the result holds, per segment, the row of its last token (scoreRows / topnRows / sampleNucleus read rows).  In the
    // host-authoritative mode every slot is pushed before and pulled after.
    struct Segment { unsigned slot; std::vector<unsigned long long> tokens; };
    std::vector<unsigned long long> forwardSegments(const std::vector<Segment> &segments)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        std::vector<rwkv_segment> segs;
        std::vector<uint64_t> ids;
        for (const Segment &s : segments) {
            segs.push_back(rwkv_segment{s.slot, (uint32_t)s.tokens.size()});
            ids.insert(ids.end(), s.tokens.begin(), s.tokens.end());
        }
        std::vector<uint64_t> last(segs.size());
        if (!residentState) pushState();
        rwkv_detail::check(rwkv_forward_segments(ctx_, ids.data(), segs.data(), segs.size(), 0, last.data()));
        if (!residentState) pullState();
        return std::vector<unsigned long long>(last.begin(), last.end());
    }
    // constrained decoding on the device (rwkv_mi355x.h "constrained decoding"): a token-level automaton in CSR form -- compiled from a regex,
    // a grammar or a choice list by a library of the caller's; include/rwkv_sampler.h constraint_trie builds the choice-list case -- and a sparse
    // logit bias per stream decide what may be generated at all.  setConstraint validates, uploads and puts every slot's automaton state to 0.
    struct Automaton { std::vector<unsigned> row_ptr, tok, next; };      // the edges of state q: row_ptr[q] .. row_ptr[q + 1]; no edges: terminal
    struct Bias { std::vector<unsigned> tok; std::vector<float> val; };  // ids strictly ascending, 1 .. 50276; finite or -inf (-inf bans the id)
    void setConstraint(const Automaton &a)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (a.row_ptr.empty() || a.tok.size() != a.next.size()) throw std::runtime_error("an automaton needs row_ptr [S + 1] and as many next as tok");
        const rwkv_automaton ra{(uint32_t)(a.row_ptr.size() - 1), 0u, (uint64_t)a.tok.size(), a.row_ptr.data(), a.tok.data(), a.next.data()};
        rwkv_detail::check(rwkv_constraint_set(ctx_, &ra));
    }
    void clearConstraint() { rwkv_detail::check(rwkv_constraint_clear(ctx_)); }
    // one constrained draw from logits row `row` of the last forward under the automaton state of slot `slot` (u: the nucleus pick's uniform);
    // advance: the slot's state moves along the pick.  Returns (token, the slot's state on return)
    std::pair<unsigned long long, unsigned> pickConstrained(const Pick &pick, const Bias &bias = Bias{}, double u = 0.0, bool advance = true,
                                                            unsigned long long row = 0, unsigned long long slot = 0, bool update = false)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (bias.tok.size() != bias.val.size()) throw std::runtime_error("a bias list needs as many values as ids");
        rwkv_pick p{};
        p.kind = pick.kind; p.temp = pick.temp; p.tau = pick.tau;
        p.nucleus = nucleusParams(pick.s, update ? RWKV_NUCLEUS_UPDATE : 0u);
        const rwkv_bias b{(uint32_t)bias.tok.size(), 0u, bias.tok.data(), bias.val.data()};
        uint64_t tok = 0;
        uint32_t q = 0;
        rwkv_detail::check(rwkv_pick_constrained(ctx_, row, slot, &p, bias.tok.empty() ? nullptr : &b, u, advance ? 1 : 0, &tok, &q));
        return {tok, q};
    }
    // decodeBatchUntil under the constraint: stream s starts in start[s] (empty: in the slot's current state) with the bias list bias[s] (empty:
    // none) and also ends where its automaton reaches a terminal state (reason RWKV_STOP_CONSTRAINT).  state[s]: the slot's automaton state after
    // consuming the stream's len[s] tokens
    struct Constrained { Until until; std::vector<unsigned> state; };
    Constrained decodeConstrained(const std::vector<unsigned long long> &first, unsigned long long n, const Pick &pick,
                                  const std::vector<unsigned long long> &seeds)
    {
        return decodeConstrained(first, n, pick, seeds, Stop(), {}, {});      // no stops, the slots' current states, no bias
    }
    Constrained decodeConstrained(const std::vector<unsigned long long> &first, unsigned long long n, const Pick &pick,
                                  const std::vector<unsigned long long> &seeds, const Stop &stop, const std::vector<unsigned> &start,
                                  const std::vector<Bias> &bias = {})
    {
        if (!start.empty() && start.size() != first.size()) throw std::runtime_error("need one start state per stream");
        if (!bias.empty() && bias.size() != first.size()) throw std::runtime_error("need one bias list per stream");
        std::vector<uint32_t> bptr(1, 0u), btok;
        std::vector<float> bval;
        btok.reserve(1); bval.reserve(1);      // (all lists empty: the arrays are still there)
        for (const Bias &b : bias) {
            if (b.tok.size() != b.val.size()) throw std::runtime_error("a bias list needs as many values as ids");
            btok.insert(btok.end(), b.tok.begin(), b.tok.end()); bval.insert(bval.end(), b.val.begin(), b.val.end());
            bptr.push_back((uint32_t)btok.size());
        }
        Constrained r;
        r.state.resize(first.size());
        const rwkv_constrain_params cp{start.empty() ? nullptr : start.data(), bias.empty() ? nullptr : bptr.data(), bias.empty() ? nullptr : btok.data(),
                                       bias.empty() ? nullptr : bval.data(), r.state.data(), 0};
        r.until = until_call(first, n, pick, seeds, stop, nullptr, &cp);
        return r;
    }
private:
    // decodeBatchUntil, with `lp` decodeBatchLogprobs and with `cp` decodeConstrained: one preparation of the C ABI's records, one push / pull of
    // host-authoritative state
    Until until_call(const std::vector<unsigned long long> &first, unsigned long long n, const Pick &pick,
                     const std::vector<unsigned long long> &seeds, const Stop &stop, const rwkv_logprob_out *lp, const rwkv_constrain_params *cp = nullptr)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (pick.kind != RWKV_PICK_GREEDY && seeds.size() != first.size()) throw std::runtime_error("need one seed per stream");
        if (!stop.max_new.empty() && stop.max_new.size() != first.size()) throw std::runtime_error("need one budget per stream");
        std::vector<uint64_t> ft(first.begin(), first.end()), sd(seeds.begin(), seeds.end()), ids(first.size() * n), flat;
        std::vector<uint32_t> lens, len(first.size()), reason(first.size());
        for (const auto &q : stop.sequences) { lens.push_back((uint32_t)q.size()); flat.insert(flat.end(), q.begin(), q.end()); }
        rwkv_pick p{};
        p.kind = pick.kind; p.temp = pick.temp; p.tau = pick.tau; p.typical_flags = pick.recipe ? RWKV_SAMPLE_RECIPE : 0;
        p.nucleus = nucleusParams(pick.s, stop.keep ? RWKV_NUCLEUS_KEEP : 0u);
        const rwkv_stop_params sp{flat.data(), lens.data(), (uint32_t)lens.size(), stop.keep ? RWKV_STOP_KEEP : 0u,
                                  stop.max_new.empty() ? nullptr : stop.max_new.data(), 0};
        Until r;
        uint64_t ran = 0;
        if (!residentState) pushState();      // host state is authoritative: continue from it ...
        const uint64_t *sdp = pick.kind == RWKV_PICK_GREEDY ? nullptr : sd.data();
        rwkv_detail::check(cp ? rwkv_decode_batch_constrained(ctx_, ft.data(), ft.size(), n, &p, sdp, cp, &sp, lp, ids.data(), len.data(), reason.data(), &ran)
                           : lp ? rwkv_decode_batch_logprobs(ctx_, ft.data(), ft.size(), n, &p, sdp, &sp, lp, ids.data(), len.data(), reason.data(), &ran)
                              : rwkv_decode_batch_until(ctx_, ft.data(), ft.size(), n, &p, sdp, &sp, ids.data(), len.data(), reason.data(), &ran));
        if (!residentState) pullState();      // ... and leave every slot where its stream stopped
        r.ids.assign(ids.begin(), ids.end()); r.len.assign(len.begin(), len.end()); r.reason.assign(reason.begin(), reason.end()); r.steps_run = ran;
        return r;
    }
public:
    // the occurrence counts of one slot (50277 floats): save / restore a session, or upload a prompt's counts; empty = zero them
    void setPenaltyCounts(unsigned long long slot, const std::vector<float> &counts)
    {
        if (!counts.empty() && counts.size() != 50277) throw std::runtime_error("need 50277 counts");
        rwkv_detail::check(rwkv_penalty_set(ctx_, slot, counts.empty() ? nullptr : counts.data()));
    }
    std::vector<float> getPenaltyCounts(unsigned long long slot)
    {
        std::vector<float> counts(50277);
        rwkv_detail::check(rwkv_penalty_get(ctx_, slot, counts.data()));
        return counts;
    }
    // copy state slot src into slot dst (fork a prefilled prompt); the host copy too when it is the authoritative one
    void copyState(unsigned long long dst, unsigned long long src)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        rwkv_detail::check(rwkv_state_copy(ctx_, dst, src));
        if (!residentState) { RWKVState sub = state->getSubState(src); state->setSubState(sub, dst); }
    }
    // scoring on the device (rwkv_mi355x.h "scoring"): log-probability (f64 log-softmax), entropy in nats and argmax per query, without
    // the 201 KB logits download per position
    struct Scores { std::vector<double> logprob, entropy; std::vector<unsigned long long> argmax; };
    // query i = (logits row rows[i] of the last forward, target id targets[i]); logits and state stay as they are
    Scores scoreRows(const std::vector<unsigned long long> &rows, const std::vector<unsigned long long> &targets)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (rows.size() != targets.size()) throw std::runtime_error("need one target per query");
        return score_call(rwkv_score_rows, rows, targets);
    }
    // feed `tokens` in GPT mode from the current state (any length: pieces of maxContext tokens, as loadContext runs them) and score
    // targets[t] under the logits that follow tokens[t].  In the host-authoritative mode slot 0 is pushed before and pulled after.
    Scores score(const std::vector<unsigned long long> &tokens, const std::vector<unsigned long long> &targets)
    {
        if (!ready) throw std::runtime_error("RWKV not loaded");
        if (tokens.size() != targets.size()) throw std::runtime_error("need one target per token");
        if (!residentState) rwkv_detail::check(rwkv_set_state(ctx_, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, 1));
        Scores s = score_call(rwkv_score, tokens, targets);
        if (!residentState) rwkv_detail::check(rwkv_get_output(ctx_, nullptr, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, 1));
        return s;
    }
    // a document: doc[0 .. m - 1) fed against doc[1 .. m)
    Scores score(const std::vector<unsigned long long> &doc)
    {
        if (doc.size() < 2) throw std::runtime_error("a document of at least two tokens");
        return score(std::vector<unsigned long long>(doc.begin(), doc.end() - 1), std::vector<unsigned long long>(doc.begin() + 1, doc.end()));
    }
    rwkv_ctx *handle() { return ctx_; }

    ~RWKV()
    {
        delete[] out;
        if (ctx_) rwkv_free(ctx_);
        delete[] tensors;
        delete state;
    }

private:
    rwkv_ctx *ctx_ = nullptr;
    int device_ = 0;
    template <typename T> static std::vector<long long> widen(const std::vector<T> &v) { return std::vector<long long>(v.begin(), v.end()); }
    Scores score_call(int (*fn)(rwkv_ctx *, const uint64_t *, const uint64_t *, uint64_t, double *, double *, uint64_t *),
                      const std::vector<unsigned long long> &first, const std::vector<unsigned long long> &targets)
    {
        const std::vector<uint64_t> a(first.begin(), first.end()), g(targets.begin(), targets.end());
        std::vector<uint64_t> am(a.size());
        Scores s;
        s.logprob.resize(a.size()); s.entropy.resize(a.size());
        rwkv_detail::check(fn(ctx_, a.data(), g.data(), a.size(), s.logprob.data(), s.entropy.data(), am.data()));
        s.argmax.assign(am.begin(), am.end());
        return s;
    }
    // slot 0 of the host-authoritative state to the device and back (nothing in the resident mode)
    void push_slot0() { if (!residentState) rwkv_detail::check(rwkv_set_state(ctx_, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, 1)); }
    void pull_slot0() { if (!residentState) rwkv_detail::check(rwkv_get_output(ctx_, nullptr, state->statexy, state->stateaa, state->statebb, state->statepp, state->statedd, 1)); }
    void ensure_ctx()
    {
        if (!ctx_) rwkv_detail::check(rwkv_create(&ctx_, device_));
    }
};

#endif // RWKV_H
