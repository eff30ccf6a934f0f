"""GPU: the load stage of polar_list_trace under the rule "Input rows" of include/polar_hip.h: rows of double or float, in an
f64 or an f32 context, as LLRs or as y with sigma, starting 0, 1 or 2 elements into a 16-byte-aligned allocation whose every
other element is NaN -- the forms and the placement of tests/input_forms.py, on one case of the one-wavefront kernel and one of
the wide kernel.  The five outputs equal tests/trace_model.py on the working LLRs the rule forms (form_rows), by ==, and the
allocation is unchanged afterwards."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import input_forms as IF  # noqa: E402
import trace_cases as TC  # noqa: E402
import trace_model as TM  # noqa: E402

NAMES = ["n64-crc6-l4", "wide-n64-l64"]
PICK = np.r_[0:12, 96, 97]           # twelve frames of the pool and the two planted rows
OUTS = ("loss_leaf", "loss_rank", "rank", "chosen", "flags")
_DECS = {}


def _values(name, form):
    """what the caller hands in: the pool's LLRs, or y values whose LLRs under the rule are of the same size"""
    llr = TC.pool(name)[1][PICK]
    return llr if form.sigma == 0 else llr * (form.sigma * form.sigma / 2)


@pytest.fixture(scope="module")
def decs():
    yield _DECS
    for d in _DECS.values():
        d.close()
    _DECS.clear()


@pytest.mark.parametrize("form", IF.FORMS, ids=IF.form_id)
@pytest.mark.parametrize("name", NAMES)
def test_trace_reads_its_rows_by_the_rule(name, form, decs):
    import torch
    kind, N, K, L, taps, seed = TC.CASES[name]
    io, dyn, crc = TC.case_code(name)
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    u = TC.pool(name)[0][PICK]
    x = np.ascontiguousarray(_values(name, form).astype(IF.NP[form.IN]))
    work = IF.form_rows(x, form.IN, form.sigma, form.R)
    want = TM.trace_model(frozen, dyn, work.astype(np.float64), u, L, crc=crc, dtype=IF.NP[form.R])
    assert (want[0] < N).any() and (want[0] == N).any()                    # lost frames and kept ones
    key = (name, form.R)
    if key not in decs:
        decs[key] = TC.decoder(name, 1 if form.R == "f32" else 0)
    dec = decs[key]
    p = IF.place(x, form.shift, "torch")
    assert IF.address(p.rows) % 16 == (form.shift * x.itemsize) % 16
    d_u = torch.from_numpy(TM.pack(u).view(np.int32)).cuda()
    t = dec.trace_list_device(p.rows, d_u, sigma=form.sigma)
    dec.synchronize()
    kinds = (np.int32, np.uint32, np.int32, np.int32, np.uint32)
    for g, k, w, n in zip(t, kinds, want, OUTS):
        assert np.array_equal(g.cpu().numpy().view(k), w), (name, IF.form_id(form), n)
    assert IF.frame_intact(p, x)


def test_the_y_form_is_told_from_a_rule_without_sigma():
    """the reference can tell: on the y values, LLRs formed without sigma give another trace in some frame"""
    name = NAMES[0]
    kind, N, K, L, taps, seed = TC.CASES[name]
    io, dyn, crc = TC.case_code(name)
    frozen = np.ones(N, dtype=np.uint8)
    frozen[io] = 0
    u, llr = TC.pool(name)[0], TC.pool(name)[1]
    y = llr * (IF.SIGMA * IF.SIGMA / 2)
    a = TM.trace_model(frozen, dyn, IF.form_rows(y, "f64", IF.SIGMA, "f64"), u, L, crc=crc)
    b = TM.trace_model(frozen, dyn, IF.wrong_rows(y, IF.SIGMA, "no sigma"), u, L, crc=crc)
    assert any(not np.array_equal(p, q) for p, q in zip(a, b))
