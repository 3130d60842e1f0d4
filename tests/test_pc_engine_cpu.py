"""The premises of the fix phase_change engine cases (tests/pc_engine_util.py), on the oracle
alone: each case reaches what tests/test_gpu_pc_engine.py holds the engine to there -- the
ENERGY threshold, Tt and Tc deciding, the retry ladder and its give-up exit between walls,
three types, calls every other step, two ranks, both halves of a restart.  A case whose
premise fails is a broken case (mend its seed, dr, rate or Tt), never a skipped one."""
import dataclasses

import numpy as np
import pytest

import c5_util
import pc_engine_util as pcu


def test_case_table():
    assert len(pcu.CASES) == len(set(pcu.CASES)) == 12
    for name in pcu.CASES:
        s, ph, steps = pcu.case(name)
        assert ph.pc is not None and 1 <= steps <= pcu.MAX_STEPS
        assert s.n in (512, 343, 144), (name, s.n)


@pytest.mark.parametrize("name", pcu.CASES)
def test_premises(po, name):
    out = pcu.premises(name)
    print(f"[pc engine] {name}: {out}")
    assert out["ninserted"] >= 1


class _Recorder:
    """stands in for the engine module: notes what the builders hand to it"""

    def __init__(self):
        self.calls = []

    def make_config(self, *a, **k):
        return ("cfg", a, k)

    def Engine(self, cfg):
        rec = self

        class E:
            def __getattr__(self, name):
                def call(*a, **k):
                    rec.calls.append((name, a, k))
                return call
        return E()


def _norm(v):
    if isinstance(v, np.ndarray):
        return ("nd", v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, (tuple, list)):
        return tuple(_norm(x) for x in v)
    if isinstance(v, dict):
        return tuple(sorted((k, _norm(x)) for k, x in v.items()))
    return v


def test_builder_matches_mp_engine_on_todays_dict():
    """pc_engine on a dict without energy_chance / rate / maxattempt makes the calls
    mp_engine makes, in order, up to Engine.phase_change's own defaults for the three"""
    from scenarios import bubble_physics, bubble_system
    s = bubble_system(8)
    ph = dataclasses.replace(bubble_physics(8, prob=0.3, Tt=-1.0, nevery=3), sortfreq=5)
    a, b = _Recorder(), _Recorder()
    c5_util.mp_engine(a, s, ph)
    pcu.pc_engine(b, s, ph)
    assert [c[0] for c in a.calls] == [c[0] for c in b.calls]
    for (na, aa, ka), (nb, ab, kb) in zip(a.calls, b.calls):
        if na == "phase_change":
            assert _norm(aa) == _norm(ab)
            assert kb == dict(ka, energy_chance=0, rate=0.0, maxattempt=10)
        else:
            assert (_norm(aa), _norm(ka)) == (_norm(ab), _norm(kb)), na
    full = pcu.with_pc(ph, energy_chance=1, rate=2.5, maxattempt=3)
    c = _Recorder()
    pcu.pc_engine(c, s, full)
    k = [x for x in c.calls if x[0] == "phase_change"][0][2]
    assert (k["energy_chance"], k["rate"], k["maxattempt"]) == (1, 2.5, 3)
