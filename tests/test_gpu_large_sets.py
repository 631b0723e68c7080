"""The weight-gradient phase's point splits held to the lattice reference at the point counts it is tuned for.

tests/test_gpu_lattice.py stops at lattice_cases.N_MAX = 1100 points, where the phase makes at most 5 point splits of the
tile launch and 9 of the skinny launch.  Here the first B lattice points of a case are the LIVE rows of a set of N rows,
15,300 to 327,700; every other row is a filler with d_out = 0 (tests/large_set_cases.py).  Fillers run the whole forward
and fill every stash; every seed the backward forms for them is exactly zero.  The gradient of the N rows is therefore
the gradient of the B live points - the float64 reference, the bit-equality classes and the bounds of
test_gpu_lattice._ref(name, B), unchanged - while the N rows are cut into the splits, slabs, rounds and reduce iterations
of a real call (large_set_cases' docstring has the counts per case, type and size).  A split whose slab is dropped, added
twice or read from the wrong slot, a live row paired with its neighbour's seed across a split boundary, a pad row that
is not silent, a reduce loop that stops one short: each changes integers.

Nothing here reads the stash; everything goes through the module's forward / backward, one of each per run."""
import pytest
import torch

import lattice_cases as LC
import large_set_cases as LS
import test_gpu_lattice as TL
from test_gpu_parity import diag, DEV
from test_gpu_half_invariants import _fault_word

pytestmark = pytest.mark.gpu

_FWD = {}


def _forward_ref(name):
    """Reference output rows and their tolerance for ALL of a case's points (the fillers cycle through them), made once."""
    if name not in _FWD:
        case = LC.get_case(name)
        bk = LC.forward_book(case, LC.N_MAX)
        out = LC.reference_out(case, LC.N_MAX, bk)
        _FWD[name] = (out, TL._forward_tolerance(case, bk, out))
    return _FWD[name]


def _run(model, case, pts, coef):
    """One training forward and one backward of sum(out * coef) -> (output rows, {name: gradient}), float64 on the host."""
    xyz, dirs, t = pts
    model.zero_grad(set_to_none=True)
    t_in = None if t is None else t.clone().requires_grad_(True)
    out = TL._call(model, case, (xyz, dirs, t_in))
    (out * coef).sum().backward()
    G = {k: (torch.zeros_like(v) if v.grad is None else v.grad).double().cpu() for k, v in model.named_parameters()}
    if t_in is not None:
        G["d_t_embed"] = t_in.grad.double().cpu()
    model.zero_grad(set_to_none=True)
    return out.detach().double().cpu(), G


def _label(case, dtype, N):
    w, s, rounds = LS.split_counts(case, dtype, N)
    return f"{w} tile-launch splits, {s} skinny splits, {rounds} round(s) by the restatement"


@pytest.mark.parametrize("pattern", LS.PATTERNS)
@pytest.mark.parametrize("dtype", LS.DTYPES)
@pytest.mark.parametrize("name,size", LS.case_sizes())
def test_live_points_in_a_large_set_have_the_reference_gradient(name, size, dtype, pattern):
    """N rows, B of them live (large_set_cases.SIZES, embed): one module forward, one backward, then a second of each.

    Forward: row j against reference row src[j], element-wise inside test_gpu_lattice._forward_tolerance - a row's operations
    do not depend on the rows around it, so the count of test_forward_is_the_float64_reference holds as it stands.  This
    is the forward's tile walk over 120 .. 5,121 row tiles.

    Gradients: test_gpu_lattice._check_gradients against _ref(name, B): torch.equal for the 16-bit exact classes,
    |G - G64| <= u (A_K + n A_1) for the others with n = _n_extra(case, B, dtype), B the LIVE count.  No rounding is added
    for the splits: a filler's term is an exact zero (+0 or -0), x + 0 = x does not round, and a sum of B non-zero terms
    and any number of zeros has at most B - 1 roundings however the splits, slabs and reduce loops group it; the adds after
    the sums (sum x power-of-two scale, the chained job, the += into the gradient) are those _n_extra already counts.

    d_t_embed (--beta): live rows like every other gradient; filler rows exactly 0 in every mode.

    Then the device fault word is 0, and a second forward / backward on the same model gives torch.equal gradients: the
    slab workspace of a call this size is reused, and nothing of the first call may leak into the second."""
    case = LC.get_case(name)
    N, B, _ = LS.SIZES[size]
    r = TL._ref(name, B)
    model = TL._model(name, dtype)
    pts64, coef64, live, src = LS.embed(case, B, N, pattern)
    pts = tuple(None if a is None else a.float().to(DEV) for a in pts64)
    coef = coef64.float().to(DEV)
    tag = f"{name} {dtype} {size} N={N} B={B} {pattern}"
    diag(f"large set {tag}: {_label(case, dtype, N)}")
    out, G = _run(model, case, pts, coef)

    # forward
    ref_out, ref_tol = _forward_ref(name)
    want, tol = ref_out[src], ref_tol[src]
    assert out.shape == want.shape and bool(torch.isfinite(out).all()), f"{tag}: shape / finite"
    err = (out - want).abs()
    diag(f"large set {tag} forward: worst |err| / tolerance {float((err / tol.clamp_min(1e-300))[tol > 0].max()):.3f}")
    if not bool((err <= tol).all()):
        j, c = [int(v) for v in (err > tol).nonzero()[0]]
        raise AssertionError(f"{tag}: {int((err > tol).sum())} output values off, first at row {j} (lattice point {int(src[j])}) channel {c}: "
                             f"got {float(out[j, c])!r} want {float(want[j, c])!r}, |err| {float(err[j, c]):.3e} > {float(tol[j, c]):.3e}")

    # gradients
    Gl = dict(G)
    if "d_t_embed" in G:
        d_t = G["d_t_embed"]
        assert d_t.shape[0] == N
        filler = torch.ones(N, dtype=torch.bool)
        filler[live] = False
        nz = (d_t != 0).any(1) & filler
        assert not bool(nz.any()), f"{tag}: d_t_embed is not exactly 0 on {int(nz.sum())} filler rows, first row {int(nz.nonzero()[0])}"
        Gl["d_t_embed"] = d_t[live]
    TL._check_gradients(f"{tag} ({_label(case, dtype, N)})", dtype, Gl, r["G64"], r["A1"], r["AK"], TL._n_extra(case, B, dtype))
    assert _fault_word() == 0

    # the same call again
    _, G2 = _run(model, case, pts, coef)
    diff = [k for k in sorted(G) if not torch.equal(G[k], G2[k])]
    assert not diff, f"{tag}: a second backward on the same model differs in {diff[:6]}"
    assert _fault_word() == 0
