// beam_app.cpp -- a caller of rwkv_decode_beam and rwkv_state_permute through the drop-in include/rwkv.h: prefill one prompt on slot 0 and search
// the `width` most probable continuations on the device.  Used by tests/test_beam_cpu.py (compiles and links without a GPU) and
// tests/test_beam_gpu.py (runs).
//   beam_app <model.bin> <width> <n_steps> [stop ids ...]
//     -> per hypothesis one line "m len score  id_0 lp_0 .. id_{n-1} lp_{n-1}" (fed 100 behind the prompt 5 6 7; every double as %a, so that a
//        caller can compare bit for bit), then "beam_ok"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rwkv.h"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const unsigned width = (unsigned)strtoul(argv[2], nullptr, 10);
    const unsigned long long steps = strtoull(argv[3], nullptr, 10);
    RWKV::Beam beam;
    beam.width = width;
    for (int i = 4; i < argc; i++) beam.stop_ids.push_back(strtoull(argv[i], nullptr, 10));
    RWKV model;
    try { model.decodeBeam(100, steps, beam); return 3; } catch (const std::runtime_error &) {}
    try { model.permuteState({0, 1}); return 3; } catch (const std::runtime_error &) {}
    model.loadFile(argv[1], width + 1);
    model.loadContext(std::vector<long long>{5, 6, 7});          // prefill on slot 0 (host-authoritative mode)
    const RWKV::BeamResult r = model.decodeBeam(100, steps, beam);
    if (r.tokens.size() != width * steps || r.token_logprob.size() != width * steps || r.len.size() != width || r.score.size() != width) return 4;
    for (unsigned m = 0; m < width; m++) {
        printf("%u %u %a ", m, r.len[m], r.score[m]);
        for (unsigned long long k = 0; k < steps; k++) printf(" %llu %a", r.tokens[m * steps + k], r.token_logprob[m * steps + k]);
        printf("\n");
    }
    // the gather on its own: a rotation forth and back leaves the host-authoritative state as it was
    std::vector<unsigned> fwd(width), back(width);
    for (unsigned m = 0; m < width; m++) { fwd[m] = (m + 1) % width; back[m] = (m + width - 1) % width; }
    const RWKVState before = *model.state;
    model.permuteState(fwd);
    model.pullState();
    const unsigned long long ld = model.num_layers * model.num_embed;
    for (unsigned long long i = 0; i < ld; i++)
        if (model.state->statexy[i] != before.statexy[ld * (1 % width) + i] || model.state->statepp[i] != before.statepp[ld * (1 % width) + i]) return 5;
    model.permuteState(back);
    model.pullState();
    for (unsigned long long i = 0; i < ld * width; i++)
        if (model.state->stateaa[i] != before.stateaa[i] || model.state->statedd[i] != before.statedd[i]) return 5;
    try { model.permuteState({0, width + 1}); return 6; } catch (const std::runtime_error &) {}
    RWKV::Beam wide;
    wide.width = RWKV_MAX_BEAM + 1;
    try { model.decodeBeam(100, steps, wide); return 6; } catch (const std::runtime_error &) {}
    printf("beam_ok\n");
    return 0;
}
