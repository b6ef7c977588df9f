"""The per-row bar of tests/row_bars.py against a float64 model of the f16 split (csrc/f16split.h), on the CPU: before a kernel is held to
the bar, the bar must accept what is faithful and reject what is subtly wrong -- at the ``c`` in use and at the largest ``c`` any kernel
family may ever be given (16).  For every operand recipe of tests/test_gpu_f16x2_rows.py, written as the GEMM the kernels see:

accepted   torch's own f32 result; the split with exact accumulation; the split with one f32 accumulator rounded after each of the three
           products (hi hi, hi lo, lo hi) of a 16-wide k-step; the same rounded after each 8-wide half of a product, as the device's matrix
           instruction does;
rejected   the lo term of one operand lost everywhere; lo hi lost in ONE k-step; the smallest-scale row zeroed; the two smallest-scale rows
           swapped; one row off by a factor 1 + 1e-4;
condition  the split's own representational error (exact accumulation against float64) stays at or below rho32 of each row's scale:
           otherwise the per-tensor scale, not the kernel, would be what the bar measures -- a recipe that breaks it gets a narrower row
           range, never a wider bar."""
import pytest
import torch

import row_bars as rb

FORMS = {}


def _form(name):
    if not FORMS:
        FORMS.update({f.name: f for f in rb.gemm_forms()})
    f = FORMS[name]
    if not hasattr(f, "exact"):
        f.exact = f.finish(rb.split_model(f.a, f.b, b_exact=f.b_exact), False)
        f.f32 = f.finish(rb.split_model(f.a, f.b, accumulate="f32", b_exact=f.b_exact), True)
        f.halves = f.finish(rb.split_model(f.a, f.b, accumulate="f32-halves", b_exact=f.b_exact), True)
    return f


NAMES = ["fc forward", "fc data gradient", "conv2 forward", "conv2 data gradient", "conv2 weight gradient", "conv3 forward", "conv3 data gradient",
         "conv3 weight gradient", "conv1 weight gradient", "fc weight gradient"]


def _bar(f, got, what, c=None):
    return rb.row_bar(f"{f.name}: {what}", got, f.ref64, f.ref32, f.ref64, c=f.c if c is None else c)


def _rejected(f, got, what):
    for c in (f.c, rb.C_MAX):
        with pytest.raises(AssertionError, match="ratio|must be all zero"):
            _bar(f, got, what, c)


def test_the_recipes_are_all_modelled():
    assert sorted(f.name for f in rb.gemm_forms()) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_the_gemm_form_is_the_layer(name):
    """The operands as a GEMM, in float64, give torch's float64 layer: the model below is a model of the right operation."""
    f = _form(name)
    got = f.finish(f.a.double() @ f.b.double().t(), False)
    scale = f.ref64.abs().amax(1, keepdim=True).clamp_min(1e-300)
    assert float(((got - f.ref64).abs() / scale).max()) <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_faithful_results_are_accepted_and_the_split_represents_every_row(name):
    f = _form(name)
    rho = rb.rho32_of(f.ref32, f.ref64)
    r_own = _bar(f, f.ref32, "torch f32 itself")
    r_exact = _bar(f, f.exact, "split, exact accumulation")
    r_f32 = _bar(f, f.f32, "split, f32 accumulation")
    r_halves = _bar(f, f.halves, "split, f32 accumulation by 8-wide halves")
    print(f"{name}: rho32 {rho:.3e}; ratios: torch f32 {r_own:.2f}, split exact {r_exact:.2f}, split f32-accumulated {r_f32:.2f}, "
          f"by halves {r_halves:.2f} (c = {f.c:g})")
    assert r_own <= 1.0 + 1e-9
    # the condition on the inputs: the split's representational error at or below rho32 of EVERY row's scale
    assert r_exact <= 1.0, f"{name}: the split itself is off by {r_exact:.2f} x rho32 on its worst row: narrow the recipe's row range"


@pytest.mark.parametrize("name", NAMES)
def test_lost_lo_terms_are_rejected(name):
    f = _form(name)
    for acc in ("exact", "f32"):
        _rejected(f, f.finish(rb.split_model(f.a, f.b, accumulate=acc, drop_lo="a", b_exact=f.b_exact), acc == "f32"), f"lo(a) lost, {acc}")
        if not f.b_exact:
            _rejected(f, f.finish(rb.split_model(f.a, f.b, accumulate=acc, drop_lo="b"), acc == "f32"), f"lo(b) lost, {acc}")
        _rejected(f, f.finish(rb.split_model(f.a, f.b, accumulate=acc, drop_lohi_step=f.step, b_exact=f.b_exact), acc == "f32"),
                  f"lo hi lost in k-step {f.step}, {acc}")


@pytest.mark.parametrize("name", NAMES)
def test_wrong_rows_are_rejected(name):
    f = _form(name)
    scale = f.ref64.abs().amax(1)
    order = torch.argsort(torch.where(scale > 0, scale, torch.full_like(scale, float("inf"))))
    lo0, lo1, mid = int(order[0]), int(order[1]), int(order[len(order) // 2])
    assert scale[lo0] > 0 and scale[lo0] <= 2.0 ** -6 * scale.max(), "the recipe has no small row"
    for base, how in ((f.exact, "exact"), (f.f32, "f32"), (f.halves, "f32-halves")):
        got = base.clone()
        got[lo0] = 0.0
        _rejected(f, got, f"smallest row ({lo0}) zeroed, {how}")
        got = base.clone()
        got[[lo0, lo1]] = base[[lo1, lo0]]
        _rejected(f, got, f"rows {lo0} and {lo1} swapped, {how}")
        for row in (lo0, mid, int(order[-1])):
            got = base.clone()
            got[row] = base[row] * (1.0 + 1e-4)
            _rejected(f, got, f"row {row} times 1 + 1e-4, {how}")
