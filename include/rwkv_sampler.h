// rwkv_sampler.h -- typical sampling over the 50277 logits (host post-processing).
//
// Behavioural mirror of reference include/rwkv/sampler/typical.h:20-66, pinned to it by
// tests/test_sampler_ref_cpu.py (20 000 draws of the reference's own function per case,
// tests/golden/typical_ref.npz).  Written against <algorithm>/<random> only -- the vendored NumCpp
// the reference pulls in for this one function is not needed.
//
// What the reference COMPUTES differs from the python recipe quoted in its header comment (softmax,
// entropy H, sort by |-log p - H|, keep the smallest set whose cumulative probability reaches tau,
// p^(1/temp), draw) in two places, both visible in the 20 000-draw histograms:
//   * the cut `probs[shifted_logits > sorted_logits[cutoff]] = 0` (typical.h:50) assigns into a TEMPORARY:
//     NumCpp's NdArray::operator[](NdArray<bool>) returns a copy (NumCpp/NdArray/NdArrayCore.hpp:778-781),
//     so nothing is cut and tau has no effect;
//   * `nc::power(probs, 1.0 / _temp)` (typical.h:52) takes a uint8 exponent (NumCpp/Functions/power.hpp:68):
//     1/temp is truncated to an integer n -- temp 0.9 or 0.8 -> n = 1 (no temperature at all), temp 0.5 ->
//     n = 2, temp > 1 -> n = 0, i.e. every weight becomes 1 and the draw is uniform over all 50277 ids.
// So typical(logits, temp, tau) draws from softmax(logits)^n, n = uint8(1/temp).  A drop-in has to give the
// reference's results, so THAT is the default here (recipe = false); recipe = true (or
// -DRWKV_TYPICAL_RECIPE=1 for the plain typical() calls) gives what the comment documents.
// LIMIT of this host restatement: like the reference it forms p^(1/temp) itself, in f64, so for near-greedy temperatures the weights
// underflow -- all of them once p_max^(1/temp) < 4.9e-324 (p_max < 1e-3 at temp 0.01, say), and then typical_u() returns 0 (`last`)
// and typical() draws from an all-zero discrete_distribution; short of that, the small weights are lost first.  The device sampler
// (csrc/sampler.hip.h) forms its weights relative to the largest kept one and has no such limit; tests/sampler_cases.py holds both to a
// log-space evaluation and compares this header only where the total of its weights is a normal number.
// Off the hot path; kept because the pybind surface exposes it.
#ifndef RWKV_SAMPLER_H
#define RWKV_SAMPLER_H

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

// the generator behind typical(): seeded from the OS like nc::random's default, or from the environment variable
// RWKV_SAMPLER_SEED for reproducible runs
inline std::mt19937_64 &rwkv_sampler_rng()
{
    static std::mt19937_64 g{[] {
        const char *e = std::getenv("RWKV_SAMPLER_SEED");
        return e ? (unsigned long long)std::strtoull(e, nullptr, 10) : (unsigned long long)std::random_device{}();
    }()};
    return g;
}

#ifndef RWKV_TYPICAL_RECIPE
#define RWKV_TYPICAL_RECIPE 0
#endif

// weights of the sampling distribution (unnormalised): the part of typical() before the draw
inline std::vector<double> typical_weights(const float *_logits, float _temp, float _tau, bool recipe = RWKV_TYPICAL_RECIPE != 0)
{
    const int len = 50277;
    std::vector<double> probs(len), shifted(len);
    double mx = _logits[0];
    for (int i = 1; i < len; i++) mx = std::max<double>(mx, _logits[i]);
    double z = 0;
    for (int i = 0; i < len; i++) { probs[i] = std::exp((double)_logits[i] - mx); z += probs[i]; }
    double ent = 0;
    for (int i = 0; i < len; i++) {
        probs[i] /= z;
        const double nl = -std::log(probs[i]);
        shifted[i] = nl;
        const double t = nl * probs[i];
        if (!std::isnan(t)) ent += t;
    }
    if (recipe) {
        for (int i = 0; i < len; i++) shifted[i] = std::fabs(shifted[i] - ent);
        std::vector<int> ids(len);
        std::iota(ids.begin(), ids.end(), 0);
        std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return shifted[a] < shifted[b]; });
        double cum = 0;
        int cutoff = 0;
        for (int i = 0; i < len; i++) { cum += probs[ids[i]]; if (cum < (double)_tau) cutoff++; }
        if (cutoff >= len) cutoff = len - 1;
        const double thr = shifted[ids[cutoff]];
        for (int i = 0; i < len; i++) if (shifted[i] > thr) probs[i] = 0;
    }
    if (_temp != 1.0f) {
        if (recipe) {
            for (int i = 0; i < len; i++) probs[i] = std::pow(probs[i], 1.0 / (double)_temp);
        } else {      // nc::power(NdArray<double>, uint8): integer exponent, repeated multiplication (NumCpp/Utils/power.hpp:46-60)
            const double e = 1.0 / (double)_temp;
            const unsigned n = e >= 255.0 ? 255u : (unsigned)(unsigned char)e;
            for (int i = 0; i < len; i++) {
                double r = n == 0 ? 1.0 : probs[i];
                for (unsigned k = 1; k < n; k++) r *= probs[i];
                probs[i] = r;
            }
        }
    }
    return probs;
}

// deterministic draw for a given uniform u in [0, 1): inverse CDF in token order -- the draw the device
// sampler (csrc/sampler.hip.h, rwkv_sample_typical) makes, so the two can be compared token for token
inline int typical_u(const float *_logits, float _temp, float _tau, double u, bool recipe = RWKV_TYPICAL_RECIPE != 0)
{
    const std::vector<double> w = typical_weights(_logits, _temp, _tau, recipe);
    double total = 0;
    for (double v : w) total += v;
    const double target = u * total;
    double c = 0;
    int last = 0;
    for (int i = 0; i < (int)w.size(); i++) {
        if (w[i] > 0) { c += w[i]; last = i; if (target < c) return i; }
    }
    return last;
}

// ---- nucleus sampling with repetition penalties: the host twin of the device sampler (csrc/nucleus.hip.h; the semantics are those of
// include/rwkv_mi355x.h) as a plain sort-based restatement, the counterpart of typical_weights / typical_u.  counts: the f32 [50277]
// occurrence counts of the stream, or nullptr (none).  Weights are formed relative to the largest logit, which is always kept: no limit at
// near-greedy temperatures.
inline std::vector<double> nucleus_weights(const float *_logits, const float *counts, float _temp, float top_p, unsigned top_k,
                                           float presence = 0.f, float frequency = 0.f, bool ban0 = false)
{
    const int len = 50277;
    std::vector<double> l(len), probs(len);
    for (int i = 0; i < len; i++) {
        l[i] = _logits[i];
        if (counts && (presence != 0.f || frequency != 0.f) && counts[i] > 0.f) l[i] -= (double)presence + (double)counts[i] * (double)frequency;
    }
    if (ban0) l[0] = -99.0;
    const double mx = *std::max_element(l.begin(), l.end());
    double z = 0;
    for (int i = 0; i < len; i++) { probs[i] = std::exp(l[i] - mx); z += probs[i]; }
    for (int i = 0; i < len; i++) probs[i] /= z;
    std::vector<int> ids(len);
    std::iota(ids.begin(), ids.end(), 0);
    std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return probs[a] > probs[b]; });
    double cum = 0;
    int cutoff = 0;
    for (int i = 0; i < len; i++) { cum += probs[ids[i]]; if (cum < (double)top_p) cutoff++; }
    if (cutoff >= len) cutoff = len - 1;
    double thr = probs[ids[cutoff]];                                                  // ties at the cut are kept
    if (top_k > 0 && top_k < (unsigned)len) thr = std::max(thr, probs[ids[top_k - 1]]);
    for (int i = 0; i < len; i++) {
        const double d = l[i] - mx;
        probs[i] = probs[i] >= thr ? std::exp(_temp == 1.0f ? d : d / (double)_temp) : 0.0;
    }
    return probs;
}

// deterministic draw for a given uniform u in [0, 1): inverse CDF in token order, the draw rwkv_sample_nucleus makes
inline int nucleus_u(const float *_logits, const float *counts, float _temp, float top_p, unsigned top_k, double u,
                     float presence = 0.f, float frequency = 0.f, bool ban0 = false)
{
    const std::vector<double> w = nucleus_weights(_logits, counts, _temp, top_p, top_k, presence, frequency, ban0);
    double total = 0;
    for (double v : w) total += v;
    const double target = u * total;
    double c = 0;
    int last = 0;
    for (int i = 0; i < (int)w.size(); i++) {
        if (w[i] > 0) { c += w[i]; last = i; if (target < c) return i; }
    }
    return last;
}

// the count update behind a pick, in f32 as the device does it: counts <- f32(counts * decay), counts[pick] += 1
inline void nucleus_count(float *counts, int pick, float decay)
{
    if (decay != 1.0f)
        for (int i = 0; i < 50277; i++) counts[i] = counts[i] * decay;
    counts[pick] += 1.0f;
}

// ---- stop sequences and budgets: the host twin of the scan the device decode loops make behind every pick (csrc/stop.hip.h; the semantics
// are those of include/rwkv_mi355x.h rwkv_decode_batch_until) for ONE stream.  ids: the picks g_0 .. g_{n-1} of an n-step call fed `first`;
// stops: the stop sequences (each 1 .. 8 ids); max_new: the budget (0: none; n is none too).  history: the stream's newest ids, oldest first,
// as the previous call left them -- pass it again to continue (RWKV_STOP_KEEP: it goes on only if it ends in `first`), pass an empty one
// to start with `first`; on return it ends with the last id scanned, at most 7 long.  len = ids counted up to and including the one that
// stopped the stream (n when nothing did); reason 0 ran all n, 1 budget, 2 + j sequence j (the lowest j of several, a sequence before the budget).
struct stop_result { unsigned len, reason; };
inline stop_result stop_scan(const std::vector<unsigned long long> &ids, unsigned long long first,
                             const std::vector<std::vector<unsigned long long>> &stops, unsigned max_new,
                             std::vector<unsigned long long> &history)
{
    const size_t keep = 7;      // RWKV_STOP_MAX_LEN - 1: with the pick, the 8 ids the longest sequence covers
    if (history.empty() || history.back() != first) history.assign(1, first);
    for (size_t k = 0; k < ids.size(); k++) {
        history.push_back(ids[k]);
        unsigned reason = 0;
        for (size_t j = 0; j < stops.size() && !reason; j++) {
            const std::vector<unsigned long long> &q = stops[j];
            if (!q.empty() && q.size() <= history.size() && std::equal(q.begin(), q.end(), history.end() - (std::ptrdiff_t)q.size())) reason = 2 + (unsigned)j;
        }
        if (!reason && max_new && k + 1 == max_new && k + 1 < ids.size()) reason = 1;
        if (history.size() > keep) history.erase(history.begin(), history.end() - (std::ptrdiff_t)keep);
        if (reason) return stop_result{(unsigned)(k + 1), reason};
    }
    return stop_result{(unsigned)ids.size(), 0u};
}

// ---- beam search: the host twin of the selection the device makes behind every step (csrc/beam.hip.h k_beam_select; the semantics are those of
// include/rwkv_mi355x.h rwkv_decode_beam).  W beams; top_ids / top_lp: [W][W + 1], the top W + 1 of every row with their log-probabilities, as
// RWKV::topnRows returns them; cum [W] the cumulative scores; ended [W]; last [W] the ids the rows were fed (an ended row's end token); stops: the
// single-token stop ids.  A live row offers its W best ids other than id 0 at cum + logprob (one f64 add), an ended row its end token again at
// cum, log-prob 0; the W best become beams 0 .. W - 1: descending score, equal scores by ascending parent, then by the row's own order.  The
// order is taken on an order-preserving 64-bit image of the score, as the device takes it, so that the result is defined for every input.
struct beam_pick { unsigned parent; unsigned long long token; double score, token_logprob; bool ended; };
inline unsigned long long beam_score_key(double v)
{
    unsigned long long b = 0;
    if (v != 0.0) std::memcpy(&b, &v, 8);                 // (-0.0 is keyed as +0.0: equal scores)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline std::vector<beam_pick> beam_select(unsigned W, const unsigned long long *top_ids, const double *top_lp, const double *cum,
                                          const unsigned char *ended, const unsigned long long *last,
                                          const std::vector<unsigned long long> &stops)
{
    struct cand { unsigned long long key; beam_pick p; };
    std::vector<cand> all;                                // in (parent, row order): what a stable sort keeps among equal scores
    const unsigned n = W + 1;
    for (unsigned j = 0; j < W; j++) {
        if (ended[j]) { all.push_back(cand{beam_score_key(cum[j]), beam_pick{j, last[j] < 50277 ? last[j] : 0ull, cum[j], 0.0, true}}); continue; }
        bool has0 = false;
        for (unsigned i = 0; i < n; i++) has0 = has0 || top_ids[j * n + i] == 0;
        for (unsigned i = 0; i < n; i++) {
            const unsigned long long g = top_ids[j * n + i];
            if (g == 0 || !(has0 || i < W)) continue;
            const double lp = top_lp[j * n + i], s = cum[j] + lp;
            all.push_back(cand{beam_score_key(s), beam_pick{j, g < 50277 ? g : 0ull, s, lp, false}});
        }
    }
    std::stable_sort(all.begin(), all.end(), [](const cand &a, const cand &b) { return a.key > b.key; });
    std::vector<beam_pick> out;
    for (unsigned m = 0; m < W && m < all.size(); m++) {
        beam_pick p = all[m].p;
        p.ended = p.ended || std::find(stops.begin(), stops.end(), p.token) != stops.end();
        out.push_back(p);
    }
    return out;
}

// ---- constrained decoding: the host twins of csrc/constrain.hip.h and the ONE validator of automata and bias lists (the semantics are those of
// include/rwkv_mi355x.h rwkv_decode_batch_constrained).  An automaton is S states in CSR form -- the edges of state q are row_ptr[q] ..
// row_ptr[q + 1], tok strictly ascending inside a row, 1 .. 50276, next < S; a state without edges is terminal -- a bias list at most 300 pairs
// (id strictly ascending, 1 .. 50276; value finite or -inf).
struct constraint_automaton {
    std::vector<unsigned> row_ptr, tok, next;             // [S + 1], [nnz], [nnz]
    unsigned states() const { return row_ptr.empty() ? 0u : (unsigned)row_ptr.size() - 1u; }
};
struct constraint_view { unsigned long long S; const unsigned *row_ptr; unsigned long long nnz; const unsigned *tok, *next; };
struct bias_view { unsigned long long n; const unsigned *tok; const float *val; };
// nullptr when the automaton (a != nullptr) and the bias list (b != nullptr) are well formed, else the NAME of the first rule broken:
// "states" (S = 0 or above 4096), "edges" (nnz above 1 << 24), "row_ptr" (a NULL array, row_ptr[0] != 0 or not non-decreasing), "row_ptr_end"
// (row_ptr[S] != nnz), "tok_range" (0 or >= 50277), "tok_order" (unsorted or duplicate inside a row), "next" (>= S), "bias_count" (above 300),
// "bias_range", "bias_order", "bias_value" (NaN or +inf).  O(nnz + n).
inline const char *constraint_check(const constraint_view *a, const bias_view *b)
{
    if (a) {
        if (a->S == 0 || a->S > 4096ull) return "states";
        if (a->nnz > (1ull << 24)) return "edges";
        if (!a->row_ptr || (a->nnz && (!a->tok || !a->next)) || a->row_ptr[0] != 0u) return "row_ptr";
        for (unsigned long long q = 0; q < a->S; q++)
            if (a->row_ptr[q + 1] < a->row_ptr[q]) return "row_ptr";
        if (a->row_ptr[a->S] != a->nnz) return "row_ptr_end";
        for (unsigned long long q = 0; q < a->S; q++)
            for (unsigned e = a->row_ptr[q]; e < a->row_ptr[q + 1]; e++) {
                if (a->tok[e] == 0u || a->tok[e] >= 50277u) return "tok_range";
                if (e > a->row_ptr[q] && a->tok[e] <= a->tok[e - 1]) return "tok_order";
                if (a->next[e] >= a->S) return "next";
            }
    }
    if (b) {
        if (b->n > 300ull) return "bias_count";
        if (b->n && (!b->tok || !b->val)) return "bias_range";
        for (unsigned long long i = 0; i < b->n; i++) {
            if (b->tok[i] == 0u || b->tok[i] >= 50277u) return "bias_range";
            if (i && b->tok[i] <= b->tok[i - 1]) return "bias_order";
            if (std::isnan(b->val[i]) || b->val[i] == INFINITY) return "bias_value";
        }
    }
    return nullptr;
}
// the constrained row of logits row l under state q and bias b, bit for bit the device's (k_constrain_rows): c_i = l_i + b_i (one f32 add, b_i = 0
// where i is not listed) where q has an edge on i, -inf otherwise.  a == nullptr: the implicit state that allows every id but 0.  A TERMINAL state
// allows every id but 0 too: the row a stream keeps running on behind its end
inline void constrained_row(const float *l, const constraint_view *a, unsigned q, const bias_view *b, float *c)
{
    const int len = 50277;
    const bool all = !a || a->row_ptr[q] == a->row_ptr[q + 1];
    std::vector<unsigned char> allowed(len, all ? 1 : 0);
    allowed[0] = 0;
    for (unsigned e = all ? 0u : a->row_ptr[q]; !all && e < a->row_ptr[q + 1]; e++) allowed[a->tok[e]] = 1;
    std::vector<float> bias(len, 0.0f);
    for (unsigned long long i = 0; b && i < b->n; i++) bias[b->tok[i]] = b->val[i];
    for (int i = 0; i < len; i++) {
        volatile float sum = l[i] + bias[i];                // (one rounding to f32, whatever the host's evaluation width)
        c[i] = allowed[i] ? sum : -INFINITY;
    }
}
// the state after pick g in state q (k_constraint_advance): next[e] for the edge e of q with tok[e] == g; q itself when q has no edge on g
inline unsigned constraint_next(const constraint_view *a, unsigned q, unsigned g)
{
    const unsigned *lo = a->tok + a->row_ptr[q], *hi = a->tok + a->row_ptr[q + 1];
    const unsigned *e = std::lower_bound(lo, hi, g);
    return e != hi && *e == g ? a->next[e - a->tok] : q;
}
// The automaton that spells exactly one of the given token sequences (the multiple-choice case): a trie, shared prefixes merged, state 0 the root,
// states numbered in the order the choices first reach them, every leaf terminal.  "Exactly one of" under greedy or sampled decoding means: the
// stream ends (RWKV_STOP_CONSTRAINT) when it reaches a state WITHOUT edges.  A choice that is a proper prefix of another one ends in a state that
// has edges, so the automaton cannot end there: such a choice is accepted as a path, but a stream that follows it goes on to one of its
// extensions -- the caller ends the shorter choice with its own end-of-choice token if both must be reachable.  Empty choices and ids outside
// 1 .. 50276 are skipped.
inline constraint_automaton constraint_trie(const std::vector<std::vector<unsigned long long>> &choices)
{
    std::vector<std::vector<std::pair<unsigned, unsigned>>> kids(1);      // per state: (tok, next)
    for (const auto &ch : choices) {
        bool ok = !ch.empty();
        for (unsigned long long t : ch) ok = ok && t >= 1 && t < 50277ull;
        if (!ok) continue;
        unsigned q = 0;
        for (unsigned long long t : ch) {
            unsigned nx = 0;
            bool found = false;
            for (const auto &kv : kids[q]) if (kv.first == (unsigned)t) { nx = kv.second; found = true; }
            if (!found) { nx = (unsigned)kids.size(); kids[q].emplace_back((unsigned)t, nx); kids.emplace_back(); }
            q = nx;
        }
    }
    constraint_automaton A;
    A.row_ptr.push_back(0u);
    for (auto &k : kids) {
        std::sort(k.begin(), k.end());
        for (const auto &kv : k) { A.tok.push_back(kv.first); A.next.push_back(kv.second); }
        A.row_ptr.push_back((unsigned)A.tok.size());
    }
    return A;
}

inline int typical(float *_logits, float _temp = 0.9, float _tau = 0.8)
{
    const std::vector<double> probs = typical_weights(_logits, _temp, _tau);
    std::discrete_distribution<int> d(probs.begin(), probs.end());
    return d(rwkv_sampler_rng());
}

inline std::vector<unsigned long long> typical(int batchsize, float *_logits, float _temp = 0.9, float _tau = 0.8)
{
    std::vector<unsigned long long> out;
    for (int i = 0; i < batchsize; i++) out.push_back(typical(&_logits[i * 50277], _temp, _tau));
    return out;
}

#endif
