// segments_app.cpp -- a caller of rwkv_forward_segments through the drop-in include/rwkv.h: the step of a continuous-batching server.  Two prompts of
// different lengths are prefilled into slots 1 and 2 while the stream on slot 0 takes one decode row, all in ONE call.  Used by
// tests/test_segments_cpu.py (compiles and links without a GPU) and tests/test_segments_gpu.py (runs).
//   segments_app <model.bin>
//     -> "last r0 r1 r2" (the logits row of each segment's last token), "argmax a0 a1 a2" (of those rows, through scoreRows), then a second step
//        that feeds every stream its argmax, "last r0 r1 r2" / "argmax a0 a1 a2" again, then "segments_ok"
#include <cstdio>
#include <vector>
#include "rwkv.h"

static std::vector<unsigned long long> step(RWKV &model, const std::vector<RWKV::Segment> &segs)
{
    const std::vector<unsigned long long> last = model.forwardSegments(segs);
    const RWKV::Scores s = model.scoreRows(last, std::vector<unsigned long long>(last.size(), 1));
    printf("last");
    for (unsigned long long r : last) printf(" %llu", r);
    printf("\nargmax");
    for (unsigned long long a : s.argmax) printf(" %llu", a);
    printf("\n");
    return s.argmax;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    RWKV model;
    try { model.forwardSegments({{0, {5}}}); return 3; } catch (const std::runtime_error &) {}
    model.loadFile(argv[1], 80);
    const std::vector<unsigned long long> a = step(model, {{0, {100}}, {1, {5, 6, 7, 800, 9}}, {2, {11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22}}});
    if (a.size() != 3) return 4;
    step(model, {{2, {a[2]}}, {0, {a[0]}}, {1, {a[1]}}});        // every stream is a decode row now; the order of the segments is the caller's
    try { model.forwardSegments({{1, {5}}, {1, {6}}}); return 6; } catch (const std::runtime_error &) {}      // a slot twice
    try { model.forwardSegments({{80, {5}}}); return 6; } catch (const std::runtime_error &) {}
    try { model.forwardSegments({{0, {}}}); return 6; } catch (const std::runtime_error &) {}
    printf("segments_ok\n");
    return 0;
}
