"""The problems, mask planes and assembled references of the plan table's rows
(tests/plans.py) under max_bias / logit_softcap, computed once per session, and
the guarded launch of one of them: shared by tests/test_gpu_op_params.py and
tests/test_gpu_sinks.py.

A problem's seed is 500 + the number of entries the cache holds when the
problem is first asked for, so what a row's problem is follows from the order
in which the session's cases run.
"""
import fattn
import op_params as op
import views
from problems import make_problem

cache = {}


def problem(spec, scale=None):
    key = ("p", spec.id, scale)
    if key not in cache:
        NQ, H, Hkv, N = spec.shape
        cache[key] = make_problem(D=spec.D, NQ=NQ, H=H, Hkv=Hkv, N=N, kv_type=spec.kt, v_type=spec.vt or None,
                                  mask="none", seed=500 + len(cache), scale=scale)
    return cache[key]


def plane(spec, kind):
    NQ, _, _, N = spec.shape
    if kind == "none":
        return None
    key = ("m", kind, NQ, N)
    if key not in cache:
        cache[key] = op.distance_mask(NQ, N) if kind == "distance" else op.random_mask(NQ, N)
    return cache[key]


def reference(spec, scale, kind, **kw):
    """The assembled reference of (spec, scale, mask kind, parameters), computed once."""
    key = ("r", spec.id, scale, kind, tuple(sorted(kw.items())))
    if key not in cache:
        cache[key] = op.one_plane(problem(spec, scale), plane(spec, kind), spec.variants, **kw).reference()
    return cache[key]


def premultiplied_oracle(spec):
    """The frozen oracle over spec's problem with H head planes slope * distance mask at max_bias 8."""
    key = ("pre", spec.id)
    if key not in cache:
        cache[key] = op.premultiplied_planes(problem(spec), plane(spec, "distance"), 8.0).oracle()
    return cache[key]


def launch(spec, vp, dev, nomask=False, kernel=None):
    """vp under spec's options through views.GpuView: (describe, output)."""
    with fattn.options(dict(spec.opts)):
        g = views.GpuView(vp, dev, spec.kv_chunk)
        d = g.describe()
        want = spec.kernel if kernel is None else kernel
        if nomask:
            want = want.replace(" + pf_mask_flags", "")
        assert want in d, d
        got = g.run()
    assert g.guards_intact(), d
    return d, got
