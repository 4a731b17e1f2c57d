"""The runs of tests/floor_cases.py WITHOUT a GPU, from the reference alone: at most 2 draws of a run are excused and no surprise comes within
1e-9 max(1, mu) of mu at any Mirostat step; and the host twins minp_u / mirostat_u (tests/cpp/floor_app.cpp) agree with the reference, mu included."""
import subprocess

import pytest

import floor_cases as fc
from support import build_app


@pytest.fixture(scope="module")
def app(tmp_path_factory):
    return build_app("floor_app", tmp_path_factory.mktemp("floorc"), link=False, opt="-O2")


@pytest.mark.parametrize("label,lname,run,counted,shift,row,slot", fc.RUNS, ids=fc.IDS)
def test_caps_hold_and_host_twin_agrees(app, tmp_path, label, lname, run, counted, shift, row, slot):
    draws = fc.draws_of(lname, run, counted, shift)
    assert sum(r.excused(u) for (u, r, *_) in draws) <= fc.MAX_EXCUSED and all(d[5] is None or d[5] > fc.MARGIN for d in draws)
    lp, cp = str(tmp_path / "logits.bin"), str(tmp_path / "counts.bin") if counted else "-"
    for path, data in ((lp, fc.logits_of(lname, run.ban0)),) + (((cp, fc.counts_of(lname, shift)),) if counted else ()):
        data.tofile(path)
    args = [run.temp, run.par, run.eta, draws[0][3] or 0.0, run.presence, run.frequency, float(run.ban0)] + [d[0] for d in draws]
    out = subprocess.run([app, lp, cp, run.kind] + [repr(float(x)) for x in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and len(out.stdout.splitlines()) == len(draws), out.stderr[-2000:]
    for (u, r, want, _, mu1, _), ln in zip(draws, out.stdout.splitlines()):
        g, mu = int(ln.split()[0]), float(ln.split()[1])
        assert g == want or r.excused(u), (u, g, want)
        if g != want:
            break                   # (an excused draw: the twin's mu goes its own way from here)
        assert mu1 is None or abs(mu - mu1) <= 1e-8, (u, mu, mu1)
