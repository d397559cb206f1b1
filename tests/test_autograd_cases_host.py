"""CPU only: the references of tests/autograd_cases.py checked against each other and against the comparison rule, without a kernel.

The GPU suite compares with ``|actual - ref64| <= TOL * scale + 4 |ref32 - ref64|``.  The slack term must not be able to hide a failure, so
every tensor of every reference of every table entry has to satisfy ``4 |ref32 - ref64| <= TOL * scale`` (per entry weighted by the PNA
family's conditioning weights where the entry carries them): the slack can at most double the allowance."""
import pytest
import torch

from tests import autograd_cases as ac


def same(a, b):
    """Equal up to the order of the oracle's own sums: torch's CPU index_add visits the rows of a long scatter in thread order, so two
    evaluations of one reference may differ in the last bits.  64 ulps of the tensor's scale (8e-6 in fp32) is far inside TOL."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool(((a - b).abs().max() <= 64 * torch.finfo(a.dtype).eps * max(1.0, b.abs().max().item())) if a.numel() else True)


@pytest.mark.parametrize("name", ac.NAMES)
def test_slack_is_at_most_the_tolerance(name):
    rows = ac.slack_report(ac.get(name))
    assert rows
    bad = [f"{what}: 4 * gap {slack:.3e} > TOL * scale {allowed:.3e}" for what, slack, allowed in rows if not slack <= allowed]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ac.NAMES)
def test_frozen_reference_equals_baseline_on_shared_tensors(name):
    c = ac.get(name)
    for dt in (torch.float32, torch.float64):
        outs, grads = ac.reference(c, dt)
        assert all(grads[k] is not None and grads[k].shape == c.inputs[k].shape for k in c.diff)
        for need in c.subsets():
            o, g = ac.reference(c, dt, need)
            assert all(same(a, b) for a, b in zip(o, outs))
            for k in c.diff:
                if k in need:
                    assert same(g[k], grads[k]), f"{name}: d{k} with only {sorted(need)} requiring grad"
                else:
                    assert g[k] is None


@pytest.mark.parametrize("name", ac.NAMES)
def test_twice_run_reference_is_exactly_double(name):
    c = ac.get(name)
    for dt in (torch.float32, torch.float64):
        once, twice = ac.reference(c, dt)[1], ac.reference(c, dt, times=2)[1]
        for k in c.diff:
            assert same(twice[k], 2 * once[k]), f"{name}: d{k}"


@pytest.mark.parametrize("name", [n for n in ac.NAMES if "partial_full" not in ac.get(n).na])
def test_partial_then_full_reference_equals_fresh(name):
    c = ac.get(name)
    for dt in (torch.float32, torch.float64):
        fresh, after = ac.reference(c, dt)[1], ac.reference_partial_then_full(c, dt)
        for k in c.diff:
            assert same(after[k], fresh[k]), f"{name}: d{k}"


def test_unused_output_references_are_none_where_no_path_exists():
    """Only the pass-through output used: no gradient reaches the attention or the weights, and dx is the upstream gradient itself."""
    for name in ac.NAMES:
        c = ac.get(name)
        if not name.endswith("_passthrough"):
            continue
        _, g = ac.reference(c, torch.float64, used=(False, True))
        assert torch.equal(g["x"], c.gouts(torch.float64)[1])
        assert all(g[k] is None for k in c.diff if k != "x")


def test_every_pattern_applies_or_says_why_not():
    assert len(set(ac.NAMES)) == len(ac.NAMES)
    for name in ac.NAMES:
        c = ac.get(name)
        assert set(c.na) <= set(ac.PATTERNS)
        assert all(isinstance(r, str) and r for r in c.na.values())
        assert set(c.layouts) <= set(c.diff) and set(c.weights) <= set(c.diff) and set(c.other_launch) <= set(c.diff)
    cases = ac.pattern_cases()
    assert len(cases) == len(set(cases))
    assert {p for p, _, _ in cases} == set(ac.PATTERNS)


def test_redraws_are_needed():
    """A recorded redraw is the FIRST draw that meets the slack condition: every earlier one misses it."""
    for name, draw in ac.REDRAW.items():
        for earlier in range(draw):
            saved = dict(ac.REDRAW)
            try:
                ac.REDRAW[name] = earlier
                ac._REFS.clear()
                rows = ac.slack_report(ac.BUILDERS[name](name))
            finally:
                ac.REDRAW.clear()
                ac.REDRAW.update(saved)
                ac._REFS.clear()
            assert any(slack > allowed for _, slack, allowed in rows), f"{name}: draw {earlier} already passes"
