"""one rwkv_forward call on a long prompt (passes of RWKV_SEQ_ROWS = 64 or 32 rows as a software pipeline over RWKV_SEQ_STAGES streams) and a 96-stream batched
step: python tools/long_prompt_bench.py [model] [tokens]
--digest: no timing; per prompt length in `tokens` (a comma-separated list) one rwkv_forward from the zero state, then the 96-stream step, and the
SHA-256 of the logits and of the five state arrays each call leaves -- to compare two builds of the engine (RWKV_LIB) bit for bit"""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch                                                 # noqa: E402
from rwkv_cpp_accelerated_amd import engine, modelfile as mf              # noqa: E402

digest = "--digest" in sys.argv
argv = [a for a in sys.argv if a != "--digest"]
model = argv[1] if len(argv) > 1 else "7B"
Ts = [int(t) for t in argv[2].split(",")] if len(argv) > 2 else [512]
T = Ts[0]
L, D = mf.SHAPES[model]
m = engine.RWKV(resident=True)
m.loadTensors(L, D, mf.synthetic_tensors_torch(L, D, seed=0), maxGPT=max(Ts + [96]))
toks = [int(v) for v in np.random.default_rng(3).integers(2, mf.VOCAB, max(Ts))]


def sha(call, rows, slots):
    """logits of `rows` rows and state slots [0, slots) after `call`, as one line of digests"""
    logits = np.array(call()[: rows * mf.VOCAB])
    m.pull_state(slots)
    n = slots * L * D
    return " ".join(f"{k} {hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]}"
                    for k, a in [("logits", logits)] + [(f"state{i}", a[:n]) for i, a in enumerate(m.state.arrays())])


if digest:
    env = " ".join(f"{k}={os.environ[k]}" for k in ("RWKV_SEQ_B", "RWKV_SEQ_STAGES", "RWKV_SEQ_ROWS") if k in os.environ)
    for t in Ts:
        m.reset_state()
        print(f"digest {model} GPT {t} tokens {env}: " + sha(lambda: m.forward(toks[:t], engine.MODE_GPT), t, 1), flush=True)
    print(f"digest {model} PARRALEL 96 streams {env}: " + sha(lambda: m.forward((toks * 96)[:96], engine.MODE_PARRALEL), 96, 96), flush=True)
    m.close()
    sys.exit(0)
toks = toks[:T]
m.forward(toks, engine.MODE_GPT)
best = 1e9
for _ in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter(); m.forward(toks, engine.MODE_GPT); torch.cuda.synchronize()
    best = min(best, time.perf_counter() - t0)
par = (toks * (96 // max(1, len(toks)) + 1))[:96]
m.forward(par, engine.MODE_PARRALEL)
bp = 1e9
for _ in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(4): m.forward(par, engine.MODE_PARRALEL)
    torch.cuda.synchronize(); bp = min(bp, (time.perf_counter() - t0) / 4)
print(f"{model} RWKV_SEQ_STAGES={os.environ.get('RWKV_SEQ_STAGES', 'default')}: {T}-token prompt {T / best:.0f} tok/s ({best * 1e3:.2f} ms); 96-stream step {96 / bp:.0f} tok/s ({bp * 1e3:.2f} ms)")
m.close()
