"""The raw field entry points on the point-set forms the training step uses, held to the xyz form that the exact tests pin.

test_gpu_half_invariants.py (P1 - P3) and test_gpu_lattice.py hold the field kernels by value, but through one shape of call:
the module's forward / backward on an `xyz` array, one block, one stash, BN_BWD_ALL, zeroed accumulators.  The training
step (FusedTrainer._lean_body) gives the points as rays + depths, fills one output array and one stash by two forward
launches (point_offset / total_points), back-propagates once over the two-block set [z | z2] (seg1_points), accumulates
over two calls where R S is no tile multiple, and on several ranks runs the backward in parts.  An exact equivalence
between the forms carries everything the xyz form is held to over to the forms that run.

Generic (Siren) networks, properties 1 - 5: every comparison is torch.equal.  The points of tests/point_set_cases.py are
exact fp32 values of o + d z (asserted on the CPU by tests/test_point_sets_cpu.py), so the kernels' rebuild of a point from
its ray gives the bits the xyz form is handed; the point count, the stash layout and the point splits of the two forms
are the same, hence so is every summation order.

  set  R   S   G   R S   n_all  reaches
  A    16  8   5   128   208    second block starts at tile 1 (16-bit), ragged last tile, S != G
  B    32  12  7   384   608    two point splits of the 16-bit weight gradient
  C    64  10  8   640   1152   three splits, G a power of two while S is not
  D    13  5   3   65    104    R S no tile multiple: the second launch may not start there

Lattice (ReLU) networks, properties 6 - 9: forms that sum in another order cannot be bit-equal to the one-call form; on the
dyadic-lattice cases of tests/lattice_cases.py every fp32 accumulation is exact in any order, so they are held to the
float64 reference by test_gpu_lattice._check_gradients, unchanged, with n_extra raised by one per addition a form adds.

No tolerance here is taken from a run of the kernels, nothing reads the stash, and no assertion leaves a row or a tensor
out."""
import ctypes as C

import pytest
import torch

import lattice_cases as LC
import point_set_cases as PS
import test_gpu_lattice as TL
from test_gpu_parity import build_model, diag, DEV
from test_gpu_half_invariants import CASES, _cfg, _fault_word

pytestmark = pytest.mark.gpu

DTYPES = ["fp32", "bf16", "fp16"]
SENTINEL = 12345.0
GUARD = 8                      # rows of sentinel behind the last row of an output array
U = LC.U24

# (model, set, ray columns).  F = 512 stays on sets A and B; A6 is set A with 6-column rays (origin and direction only).
RAW = [("lambert_F512", "A", 11), ("lambert_F512", "B", 11),
       ("rpv_nlr_F256", "A", 11), ("rpv_nlr_F256", "B", 11), ("rpv_nlr_F256", "C", 11),
       ("rpv_nan_F64", "A", 11), ("rpv_nan_F64", "A", 6), ("rpv_nan_F64", "B", 11), ("rpv_nan_F64", "C", 11),
       ("rpv_nan_F512", "A", 11), ("rpv_nan_F512", "B", 11)]
VIEWDIR = [("viewdir_beta_F192", "A", 11), ("viewdir_beta_F192", "A", 6), ("viewdir_beta_F192", "C", 11)]
# set D: one block per call only (ray form forward and backward); its set form is refused (property 5)
ONE_BLOCK = RAW + VIEWDIR + [("rpv_nan_F64", "D", 11), ("lambert_F512", "D", 11), ("viewdir_beta_F192", "D", 11)]
MERGED = [c for c in RAW if c[1] in PS.MERGEABLE]

_MODELS, _INPUTS = {}, {}


def _ids(cases):
    return [f"{n}-{s}{'' if w == 11 else w}" for n, s, w in cases]


def _model(name, dtype):
    """(model, spec, flags) of a configuration of test_gpu_half_invariants.CASES, built once per (case, dtype)."""
    if (name, dtype) not in _MODELS:
        cfg, flags, seed = _cfg(name)
        model = build_model(cfg, seed, dtype)
        spec = model.spec(flags.get("apply_brdf", False), False, flags.get("nr_lr_on", False), flags.get("nr_an_on", False))
        _MODELS[(name, dtype)] = (model, spec, cfg)
    return _MODELS[(name, dtype)]


def _inputs(name, sname, stride):
    """Device tensors of a set for a configuration: rays, z, z2, X, dirs (None without --input_viewdir), the per-ray and
    per-point embeddings (None without --beta) and a random d_out (analytic-normal channels weighed down by 0.1 as the fuzz
    does), the same for every type."""
    key = (name, sname, stride)
    if key not in _INPUTS:
        cfg = _cfg(name)[0]
        R, S, G = PS.SETS[sname]
        rs = PS.ray_set(sname, stride)
        X, dirs = PS.set_points(rs)
        d = dict(R=R, S=S, G=G, n1=R * S, n_all=R * (S + G))
        for k in ("rays", "z", "z2"):
            d[k] = rs[k].float().contiguous().to(DEV)
        d["X"], d["dirs"] = X.float().contiguous().to(DEV), dirs.float().contiguous().to(DEV) if cfg.dir_dim else None
        d["t_ray"] = d["t_pt"] = None
        if cfg.beta:
            t = PS.ray_embedding(sname, cfg.t_dim)
            d["t_ray"] = t.contiguous().to(DEV)
            d["t_pt"] = torch.cat([t.repeat_interleave(S, 0), t.repeat_interleave(G, 0)]).contiguous().to(DEV)
        _INPUTS[key] = d
    return _INPUTS[key]


def _d_out(spec, n, seed, normals_only=False):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, spec.out_channels, generator=g)
    c = spec.ch_normal_an
    if c >= 0:
        d[:, c:c + 3] *= 0.1
    if normals_only:
        assert c >= 0
        keep = d[:, c:c + 3].clone()
        d.zero_()
        d[:, c:c + 3] = keep
    return d.contiguous().to(DEV)


def _new_out(spec, n):
    """An output array of n rows followed by GUARD rows, all sentinel: (whole, the n-row view the library is given)."""
    whole = torch.full((n + GUARD, spec.out_channels), SENTINEL, dtype=torch.float32, device=DEV)
    return whole, whole[:n]


def _new_stash(spec, n):
    from brdf_nerf_amd import functions as Fn
    return torch.zeros(Fn.field_stash_bytes(spec, n), dtype=torch.uint8, device=DEV)


def _is_sentinel(t):
    return bool((t == SENTINEL).all())


def _zero_grads(model):
    return {k: torch.zeros_like(v) for k, v in model.named_parameters()}


def _clear_folded(spec):
    for m, sv in spec.fold_grads.values():
        m.zero_()
        sv.zero_()


def _assert_same_grads(tag, got, want, used):
    """Every tensor of `want` bit for bit, every parameter the spec uses with a finite, non-zero gradient."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    bad = []
    for k in sorted(want):
        g, w = got[k], want[k]
        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(g).all()), f"{tag} {k}: non-finite"
        if k in used:
            assert float(w.abs().max()) > 0, f"{tag} {k}: the reference gradient is all zero"
        if not torch.equal(g, w):
            i = tuple(int(v) for v in (g != w).nonzero()[0])
            bad.append(f"{k}: {int((g != w).sum())} of {g.numel()} elements differ, first at {i}: got {float(g[i])!r} want {float(w[i])!r}")
    assert not bad, f"{tag}: " + "; ".join(bad[:6])


def _assert_same_rows(tag, got, want):
    assert got.shape == want.shape and bool(torch.isfinite(want).all()), f"{tag}: shape / finite reference"
    if not torch.equal(got, want):
        rows = (got != want).reshape(got.shape[0], -1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{tag}: {len(rows)} of {got.shape[0]} rows differ, first {rows[:8]}, max |diff| "
                             f"{float((got - want).abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------ raw-call helpers
def _forward_xyz(model, spec, packed, X):
    """One xyz-form launch with its own stash -> (out, stash, whole)."""
    from brdf_nerf_amd import functions as Fn
    whole, out = _new_out(spec, X.shape[0])
    stash = _new_stash(spec, X.shape[0])
    with torch.no_grad():
        Fn.field_forward_raw(spec, model.named(), packed, out, stash, xyz=X)
    return out, stash, whole


def _forward_set(model, spec, packed, first, second, n1, n_all, check=None):
    """Two launches into one output array and one stash: `first` at point_offset 0, `second` at n1.  check(out_rows,
    lo, hi): called after each launch with the rows it wrote; rows outside a launch's range must be untouched - sentinel
    before they are written, the first launch's bits afterwards - and so must the guard rows."""
    from brdf_nerf_amd import functions as Fn
    whole, out = _new_out(spec, n_all)
    stash = _new_stash(spec, n_all)
    with torch.no_grad():
        Fn.field_forward_raw(spec, model.named(), packed, out, stash, point_offset=0, total_points=n_all, **first)
        assert _is_sentinel(whole[n1:]), "the first launch wrote outside rows [0, n1)"
        rows1 = out[:n1].clone()
        if check:
            check(rows1, 0, n1)
        Fn.field_forward_raw(spec, model.named(), packed, out, stash, point_offset=n1, total_points=n_all, **second)
        assert torch.equal(out[:n1], rows1), "the second launch changed rows of the first"
        assert _is_sentinel(whole[n_all:]), "the second launch wrote behind the set"
        if check:
            check(out[n1:], n1, n_all)
    return out, stash, whole


def _backward(model, spec, packed, out, d_out, stash, grads=None, **kw):
    """field_backward_raw into zeroed accumulators (or `grads`) -> {parameter name: gradient}."""
    from brdf_nerf_amd import functions as Fn
    grads = _zero_grads(model) if grads is None else grads
    with torch.no_grad():
        Fn.field_backward_raw(spec, model.named(), grads, packed, out, d_out, stash, **kw)
    return grads


# ------------------------------------------------------------------------------------------------ 1: ray form, forward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,sname,stride", ONE_BLOCK, ids=_ids(ONE_BLOCK))
def test_ray_form_forward_is_the_xyz_form(name, sname, stride, dtype):
    """Property 1.  The reference is ONE xyz-form call on the set's points X (block 1 ray-major, then block 2) with each ray's
    d repeated per sample as `dirs` and its embedding row repeated per sample; by P1 a row of it does not depend on the
    batch.  Each block given as rays + depths (S samples per ray, then G) must reproduce its rows bit for bit:
    model.evaluate in grad mode (stash kept) and in no-grad mode (each against the xyz form in the same mode: the two
    are different kernel variants), field_forward_raw with a stash against the grad-mode reference, field_sigma against
    field_sigma.  The analytic-normal channels (bn_field_normals in ray form) are part of the rows; the view-direction
    model takes its direction from rays[:, 3:6] and, through model.evaluate only, its embedding per ray."""
    from brdf_nerf_amd import functions as Fn
    model, spec, cfg = _model(name, dtype)
    I = _inputs(name, sname, stride)
    packed = model.repack(spec)
    n1, named = I["n1"], model.named()
    blocks = [(I["z"], slice(0, n1)), (I["z2"], slice(n1, I["n_all"]))]
    n_cmp = 0
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            ref = model.evaluate(spec, packed, xyz=I["X"], dirs=I["dirs"], t_embed=I["t_pt"]).detach()
            assert ref.shape == (I["n_all"], spec.out_channels) and bool(torch.isfinite(ref).all())
            for z, rows in blocks:
                got = model.evaluate(spec, packed, rays=I["rays"], z=z, t_embed=I["t_ray"]).detach()
                _assert_same_rows(f"{name} {dtype} {sname} evaluate grad={grad} S={z.shape[1]}", got, ref[rows])
                n_cmp += got.numel()
        if grad:
            ref_train = ref
    if not cfg.beta:        # (field_forward_raw has no embedding argument)
        for z, rows in blocks:
            n = z.numel()
            whole, out = _new_out(spec, n)
            with torch.no_grad():
                Fn.field_forward_raw(spec, named, packed, out, _new_stash(spec, n), rays=I["rays"], z=z)
            assert _is_sentinel(whole[n:])
            _assert_same_rows(f"{name} {dtype} {sname} field_forward_raw S={z.shape[1]}", out, ref_train[rows])
            n_cmp += out.numel()
    with torch.no_grad():
        sig = Fn.field_sigma(spec, named, packed, xyz=I["X"])
        assert bool(torch.isfinite(sig).all()) and sig.shape == (I["n_all"],)
        for z, rows in blocks:
            _assert_same_rows(f"{name} {dtype} {sname} field_sigma S={z.shape[1]}", Fn.field_sigma(spec, named, packed, rays=I["rays"], z=z), sig[rows])
            n_cmp += z.numel()
    diag(f"point sets 1 {name} {dtype} {sname}{stride}: {n_cmp} values bitwise equal to the xyz form")
    assert _fault_word() == 0


# ------------------------------------------------------------------------------------------------ 2, 3: the set
_SET_REFS = {}


def _set_reference(name, sname, stride, dtype):
    """The one-call xyz form over X: its output rows and, per d_out, its gradients into zeroed accumulators (made once)."""
    key = (name, sname, stride, dtype)
    if key not in _SET_REFS:
        model, spec, cfg = _model(name, dtype)
        I = _inputs(name, sname, stride)
        packed = model.repack(spec)
        out, stash, whole = _forward_xyz(model, spec, packed, I["X"])
        assert _is_sentinel(whole[I["n_all"]:]) and bool(torch.isfinite(out).all())
        _SET_REFS[key] = dict(out=out.clone(), grads={})
    return _SET_REFS[key]


def _reference_grads(name, sname, stride, dtype, normals_only):
    r = _set_reference(name, sname, stride, dtype)
    if normals_only not in r["grads"]:
        model, spec, cfg = _model(name, dtype)
        I = _inputs(name, sname, stride)
        packed = model.repack(spec)
        d_out = _d_out(spec, I["n_all"], 31, normals_only)
        out, stash, _ = _forward_xyz(model, spec, packed, I["X"])     # (a fresh stash: a backward writes into it)
        r["grads"][normals_only] = (d_out, _backward(model, spec, packed, out, d_out, stash, xyz=I["X"]))
    return r["grads"][normals_only]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,sname,stride", MERGED, ids=_ids(MERGED))
def test_two_launches_fill_the_set_like_one_call(name, sname, stride, dtype):
    """Property 2.  Two forward launches (point_offset = 0 and R S, total_points = n_all) into one output array and one
    stash, in ray form as the training step issues them and in xyz form, against the one-call output row for row.  Rows
    outside a launch's range are untouched: rows [R S, n_all) and the guard rows behind the array hold the planted sentinel
    after the first launch, rows [0, R S) hold the first launch's bits after the second, the guard rows still the
    sentinel.  The stash is not inspected: property 3 shows that it is the one-call stash."""
    model, spec, cfg = _model(name, dtype)
    I = _inputs(name, sname, stride)
    ref = _set_reference(name, sname, stride, dtype)["out"]
    packed = model.repack(spec)
    n1, n_all = I["n1"], I["n_all"]
    forms = {"rays": (dict(rays=I["rays"], z=I["z"]), dict(rays=I["rays"], z=I["z2"])),
             "xyz": (dict(xyz=I["X"][:n1].contiguous()), dict(xyz=I["X"][n1:].contiguous()))}
    for form, (first, second) in forms.items():
        tag = f"{name} {dtype} {sname} {form}"
        out, _, _ = _forward_set(model, spec, packed, first, second, n1, n_all,
                                 check=lambda rows, lo, hi: _assert_same_rows(f"{tag} rows [{lo}, {hi})", rows, ref[lo:hi]))
        _assert_same_rows(tag, out, ref)
    assert _fault_word() == 0


def _an_cases(cases):
    return [(n, s, w, False) for n, s, w in cases] + [(n, s, w, True) for n, s, w in cases if CASES[n][0].get("normal") == "analystic"]


_BWD = _an_cases(MERGED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,sname,stride,normals_only", _BWD,
                         ids=[i + ("-normals" if c[3] else "") for i, c in zip(_ids([c[:3] for c in _BWD]), _BWD)])
def test_two_block_backward_is_the_xyz_backward(name, sname, stride, normals_only, dtype):
    """Property 3.  field_backward_raw(rays=, z=, z2=) over the stash the two ray-form launches filled, against the xyz-form
    backward over X on a stash of one xyz-form call: every parameter's gradient, into zeroed accumulators, with the same
    random d_out, torch.equal.  Point count, stash layout and point splits are the same, so every sum runs in the same order;
    what differs is where a kernel takes a point from - only field_adjbwd.hip (analytic normals) rebuilds x, from the ray of
    the point's OWN block (n_samples2 for the second).  For the analytic-normal models the run is repeated with d_out zero
    outside the normal channels: the adjoint backward's x is then the whole signal."""
    model, spec, cfg = _model(name, dtype)
    I = _inputs(name, sname, stride)
    d_out, want = _reference_grads(name, sname, stride, dtype, normals_only)
    packed = model.repack(spec)
    out, stash, _ = _forward_set(model, spec, packed, dict(rays=I["rays"], z=I["z"]), dict(rays=I["rays"], z=I["z2"]), I["n1"], I["n_all"])
    got = _backward(model, spec, packed, out, d_out, stash, rays=I["rays"], z=I["z"], z2=I["z2"])
    used = set(spec.used_param_names())
    if normals_only:         # the heads and the learned normal see a zero seed; the trunk and sigma carry the signal
        used = {k for k in used if k.startswith("fc_net.") and k.endswith(".weight") or k == "sigma_from_xyz.0.weight"}
    _assert_same_grads(f"{name} {dtype} {sname}{' normals only' if normals_only else ''}", got, want, used)
    assert _fault_word() == 0


# ------------------------------------------------------------------------------------------------ 4: ray form, backward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,sname,stride", ONE_BLOCK, ids=_ids(ONE_BLOCK))
def test_ray_form_backward_is_the_xyz_form(name, sname, stride, dtype):
    """Property 4.  model.evaluate(rays=, z=) + backward() against model.evaluate(xyz=, dirs=, t_embed=) + backward() on the
    same points and d_out, for block 1 (S samples per ray) and block 2 (G): every parameter's gradient torch.equal.  With
    --beta the per-ray gradient of the embedding is the xyz form's per-point gradient viewed as [R, S, t_dim] and summed
    over S - the same torch sum on what must be the same bits."""
    model, spec, cfg = _model(name, dtype)
    I = _inputs(name, sname, stride)
    packed = model.repack(spec)
    R, n1 = I["R"], I["n1"]
    used = set(spec.used_param_names())

    def run(d_out, **pts):
        model.zero_grad(set_to_none=True)
        t = pts.pop("t_embed")
        t = None if t is None else t.clone().requires_grad_(True)
        out = model.evaluate(spec, packed, t_embed=t, **pts)
        (out * d_out).sum().backward()
        g = {k: (torch.zeros_like(v) if v.grad is None else v.grad.clone()) for k, v in model.named_parameters()}
        return out.detach(), g, None if t is None else t.grad.clone()

    for z, rows in ((I["z"], slice(0, n1)), (I["z2"], slice(n1, I["n_all"]))):
        S = z.shape[1]
        tag = f"{name} {dtype} {sname} S={S}"
        d_out = _d_out(spec, R * S, 40 + S)
        X = I["X"][rows].contiguous()
        dirs = None if I["dirs"] is None else I["dirs"][rows].contiguous()
        t_pt = None if I["t_pt"] is None else I["t_pt"][rows].contiguous()
        out_x, g_x, dt_x = run(d_out, xyz=X, dirs=dirs, t_embed=t_pt)
        out_r, g_r, dt_r = run(d_out, rays=I["rays"], z=z, t_embed=I["t_ray"])
        _assert_same_rows(tag, out_r, out_x)
        _assert_same_grads(tag, g_r, g_x, used)
        if cfg.beta:
            want = dt_x.view(R, S, cfg.t_dim).sum(1)
            assert dt_r.shape == want.shape and float(want.abs().max()) > 0 and bool(torch.isfinite(want).all())
            assert torch.equal(dt_r, want), f"{tag}: d t_embed per ray differs from the per-point gradient summed over the ray's samples"
    model.zero_grad(set_to_none=True)
    assert _fault_word() == 0


# ------------------------------------------------------------------------------------------------ 5: refusals
def _backward_rc(spec, model, packed, pts, out, d_out, stash, grads, d_t=None):
    """bn_field_backward_parts on a caller-built bn_points (field_backward_raw exposes no point_offset) -> (status, message)."""
    from brdf_nerf_amd import _lib as L
    ps, gs = spec.params_struct(model.named()), spec.params_struct(grads, grads=True)
    if d_t is not None:
        gs.d_t_embed = d_t.data_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().bn_field_backward_parts(C.byref(spec.desc), C.byref(ps), p(packed), C.byref(pts), p(out), p(d_out), p(stash), C.byref(gs),
                                         L.BN_BWD_ALL, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, L.lib().bn_last_error().decode()


@pytest.mark.parametrize("dtype", DTYPES)
def test_malformed_point_sets_come_back_as_errors(dtype):
    """Property 5.  Each of these returns an error and launches nothing (the output array keeps its sentinel, the gradient
    accumulators stay zero, the device fault word stays 0): a point_offset that is no tile multiple (set D's R S = 65, and
    64 in the 16-bit modes); point_offset > 0 with total_points = 0; point_offset + n_points > total_points; a backward
    with point_offset != 0; seg1_points no multiple of n_samples; a two-block set that asks for d_t_embed."""
    from brdf_nerf_amd import functions as Fn
    from brdf_nerf_amd import _lib as L
    model, spec, cfg = _model("rpv_nan_F64", dtype)
    packed = model.repack(spec)
    named = model.named()
    tile = PS.TILE[dtype]
    D, A = _inputs("rpv_nan_F64", "D", 11), _inputs("rpv_nan_F64", "A", 11)
    n_all = A["n_all"]
    whole, out = _new_out(spec, n_all)
    stash = _new_stash(spec, n_all)
    bad_forward = [
        ("R S of set D", dict(rays=D["rays"], z=D["z2"], point_offset=D["n1"], total_points=D["n_all"])),
        ("half a tile", dict(rays=A["rays"], z=A["z2"], point_offset=tile // 2, total_points=n_all)),
        ("one row short of a tile", dict(xyz=A["X"][:16].contiguous(), point_offset=tile - 1, total_points=n_all)),
        ("offset without a set", dict(rays=A["rays"], z=A["z2"], point_offset=A["n1"], total_points=0)),
        ("past the end of the set", dict(rays=A["rays"], z=A["z2"], point_offset=A["n1"], total_points=n_all - 1)),
    ]
    assert D["n1"] % tile != 0
    for what, kw in bad_forward:
        with pytest.raises(RuntimeError, match="field"):
            with torch.no_grad():
                Fn.field_forward_raw(spec, named, packed, out, stash, **kw)
        assert _is_sentinel(whole), f"{what}: refused, but rows were written"
    # backward: a valid two-block set first, so that every pointer is a real one
    out, stash, _ = _forward_set(model, spec, packed, dict(rays=A["rays"], z=A["z"]), dict(rays=A["rays"], z=A["z2"]), A["n1"], n_all)
    d_out = _d_out(spec, n_all, 5)
    grads = _zero_grads(model)

    def refused(what, pts, sp=spec, m=model, pk=packed, o=out, d=d_out, s=stash, g=grads, d_t=None):
        rc, msg = _backward_rc(sp, m, pk, pts, o, d, s, g, d_t)
        assert rc != 0 and "field_backward" in msg, f"{what}: status {rc}, message {msg!r}"
        assert all(float(v.abs().max()) == 0.0 for v in g.values()), f"{what}: refused, but a gradient was written"
        assert all(float(a.abs().max()) == 0.0 for ent in sp.fold_grads.values() for a in ent), f"{what}: refused, but a folded gradient was written"

    _clear_folded(spec)
    refused("backward at an offset (xyz)", Fn.make_points(xyz=A["X"][tile:].contiguous(), point_offset=tile, total_points=n_all))
    pts = Fn.make_points(rays=A["rays"], z=A["z"], z2=A["z2"])
    pts.point_offset, pts.total_points = tile, n_all + tile
    refused("backward at an offset (two blocks)", pts)
    for seg1 in (A["n1"] + 1, A["n1"] - 1):
        pts = Fn.make_points(rays=A["rays"], z=A["z"], z2=A["z2"])
        pts.seg1_points = seg1
        refused(f"seg1_points = {seg1}, n_samples = {A['S']}", pts)
    assert _fault_word() == 0
    # a two-block set that asks for d_t_embed (--beta)
    mb, sb, cb = _model("viewdir_beta_F192", dtype)
    pb = mb.repack(sb)
    V = _inputs("viewdir_beta_F192", "A", 11)
    _, out_b = _new_out(sb, V["n_all"])
    stash_b = _new_stash(sb, V["n_all"])
    ps = sb.params_struct(mb.named())
    for z, off in ((V["z"], 0), (V["z2"], V["n1"])):      # (field_forward_raw has no embedding argument: the library is called as it does)
        pts = Fn.make_points(rays=V["rays"], z=z, t_embed=V["t_ray"], point_offset=off, total_points=V["n_all"])
        L.check(L.lib().bn_field_forward(C.byref(sb.desc), C.byref(ps), C.c_void_p(pb.data_ptr()), C.byref(pts), C.c_void_p(out_b.data_ptr()),
                                         C.c_void_p(stash_b.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "bn_field_forward")
    assert bool(torch.isfinite(out_b).all()) and not bool((out_b == SENTINEL).any())
    d_t = torch.full((V["n_all"], cb.t_dim), SENTINEL, dtype=torch.float32, device=DEV)
    _clear_folded(sb)
    pts = Fn.make_points(rays=V["rays"], z=V["z"], z2=V["z2"], t_embed=V["t_ray"])
    refused("d_t_embed over two blocks", pts, sb, mb, pb, out_b, _d_out(sb, V["n_all"], 6), stash_b, _zero_grads(mb), d_t)
    assert _is_sentinel(d_t)
    assert _fault_word() == 0


# ------------------------------------------------------------------------------------------------ lattice: 6 - 9
def _lattice(name, B, dtype):
    r = TL._ref(name, B)
    case = r["case"]
    model = TL._model(name, dtype)
    spec = model.spec(case.flags.get("apply_brdf", False), False, case.flags.get("nr_lr_on", False), case.flags.get("nr_an_on", False))
    return r, case, model, spec, model.repack(spec)


def _check_lattice_out(tag, r, out):
    """test_gpu_lattice's forward criterion (training forward): element-wise inside _forward_tolerance, every row."""
    got, want = out.double().cpu(), r["out"]
    tol = TL._forward_tolerance(r["case"], r["bk"], want)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), f"{tag}: shape / finite"
    err = (got - want).abs()
    if not bool((err <= tol).all()):
        i, c = [int(v) for v in (err > tol).nonzero()[0]]
        raise AssertionError(f"{tag}: {int((err > tol).sum())} output values off, first at point {i} channel {c}: got {float(got[i, c])!r} "
                             f"want {float(want[i, c])!r}, |err| {float(err[i, c]):.3e} > {float(tol[i, c]):.3e}")


def _cpu64(grads):
    return {k: v.double().cpu() for k, v in grads.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B", PS.LATTICE)
def test_lattice_set_forward_and_whole_set_backward(name, B, dtype):
    """Property 6, xyz form: two forward launches split at the tile multiple nearest B / 2 (point_offset), one backward over
    all B, d_out = the case's coefficients.  Outputs inside _forward_tolerance, gradients by _check_gradients with
    n_extra = _n_extra(case, B, dtype): the form adds no addition to the one-call form (extra additions: 0)."""
    r, case, model, spec, packed = _lattice(name, B, dtype)
    X = TL._dev_pts(case, B)[0]
    h = PS.split_point(B)
    out, stash, _ = _forward_set(model, spec, packed, dict(xyz=X[:h].contiguous()), dict(xyz=X[h:].contiguous()), h, B)
    _check_lattice_out(f"{name} {dtype} B={B} split at {h}", r, out)
    G = _backward(model, spec, packed, out, case.coef[:B].float().contiguous().to(DEV), stash, xyz=X)
    TL._check_gradients(f"{name} {dtype} B={B} set forward", dtype, _cpu64(G), r["G64"], r["A1"], r["AK"], TL._n_extra(case, B, dtype))
    assert _fault_word() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B", PS.LATTICE)
def test_lattice_gradients_accumulate_over_calls(name, B, dtype):
    """Property 7, the training step's unmerged path: two independent forward / backward pairs on the two parts of the
    batch (split at the tile multiple nearest B / 2, each with its own output array and stash) into the SAME gradient
    tensors, zero_folded=False, unfold=False on the first call and True on the second.  The result is the float64
    gradient of the whole batch by _check_gradients with n_extra = _n_extra(case, B, dtype) + 1 (extra additions: 1, the
    second call's add into a non-zero accumulator; each call's own sums are shorter than the one-call sum).
    The `+=` contract of bn_field_grads: three accumulators - one per kernel that adds into a gradient (wgrad_reduce_kernel,
    skinny_reduce_kernel, bn_unfold_heads) - are preloaded with a lattice-valued constant c and must come back as c +
    gradient.  tests/test_point_sets_cpu.py asserts that c + (first part's gradient) and c + gradient are fp32 values, so in the
    16-bit modes the tensors _check_gradients holds bit for bit still are (got - c, formed in float64, is then exact).
    The preloaded tensors it holds to the bound carry two more roundings, each relative to a partial sum of at most
    |c| + A_1: they are checked against u (A_K + (n_extra + 1) A_1) + 2 u (|c| + A_1)."""
    r, case, model, spec, packed = _lattice(name, B, dtype)
    X = TL._dev_pts(case, B)[0]
    coef = case.coef[:B].float().contiguous().to(DEV)
    h = PS.split_point(B)
    grads = _zero_grads(model)
    for k, c in PS.PRELOAD.items():
        grads[k].fill_(c)
    _clear_folded(spec)
    parts = [slice(0, h), slice(h, B)]
    for i, rows in enumerate(parts):
        Xp = X[rows].contiguous()
        out, stash, whole = _forward_xyz(model, spec, packed, Xp)
        assert _is_sentinel(whole[Xp.shape[0]:])
        _backward(model, spec, packed, out, coef[rows].contiguous(), stash, grads=grads, xyz=Xp, unfold=i == len(parts) - 1, zero_folded=False)
    _clear_folded(spec)
    G = _cpu64(grads)
    n = TL._n_extra(case, B, dtype) + 1
    rest = lambda d: {k: v for k, v in d.items() if k not in PS.PRELOAD}  # noqa: E731
    tag = f"{name} {dtype} B={B} two calls"
    TL._check_gradients(tag, dtype, rest(G), rest(r["G64"]), rest(r["A1"]), rest(r["AK"]), n)
    for k, c in PS.PRELOAD.items():
        w = r["G64"][k]
        assert bool(torch.isfinite(G[k]).all())
        if dtype != "fp32" and TL._exact_in_16_bits(k):
            assert torch.equal(G[k], w + c), f"{tag} {k}: preloaded with {c}, the accumulator is not {c} + gradient " \
                                             f"({int((G[k] != w + c).sum())} of {w.numel()} elements; overwritten: {bool(torch.equal(G[k], w))})"
        else:
            bound = U * (r["AK"][k] + n * r["A1"][k]) + 2 * U * (abs(c) + r["A1"][k])
            err = (G[k] - (w + c)).abs()
            assert bool((err <= bound).all()), f"{tag} {k}: preloaded with {c}, |accumulator - ({c} + gradient)| up to {float(err.max()):.3e}, " \
                                               f"worst ratio to the bound {float((err / bound).max()):.3e}"
    assert _fault_word() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B", PS.LATTICE)
def test_lattice_backward_in_parts(name, B, dtype):
    """Property 8.  BN_BWD_CHAIN | BN_BWD_WGRAD_TRUNK, then BN_BWD_WGRAD_HEADS | BN_BWD_SKINNY, on one stream, unfold on the
    second call: the result is the float64 gradient by _check_gradients with n_extra = _n_extra(case, B, dtype) (extra
    additions: 0 - every gradient is written by the jobs of one part).  After the first call alone every trunk gradient
    (fc_net.*) is final - torch.equal to its end value, and not zero - and every other gradient is still exactly zero, the
    folded accumulators of the heads' first layers included (a heads job that ran with the trunk's part would fill them
    early): the contract the two-bucket all-reduce of the training step relies on."""
    from brdf_nerf_amd import _lib as L
    r, case, model, spec, packed = _lattice(name, B, dtype)
    X = TL._dev_pts(case, B)[0]
    out, stash, _ = _forward_xyz(model, spec, packed, X)
    d_out = case.coef[:B].float().contiguous().to(DEV)
    grads = _zero_grads(model)
    _clear_folded(spec)
    _backward(model, spec, packed, out, d_out, stash, grads=grads, xyz=X, unfold=False, zero_folded=False, parts=L.BN_BWD_CHAIN | L.BN_BWD_WGRAD_TRUNK)
    first = {k: v.clone() for k, v in grads.items()}
    tag = f"{name} {dtype} B={B} parts"
    # (the heads' first layers are evaluated folded: what their jobs add to are the spec's folded accumulators)
    assert spec.fold_feats and set(spec.fold_grads) == {h for h, _, _ in spec.heads}
    for h, ent in spec.fold_grads.items():
        assert all(float(a.abs().max()) == 0.0 for a in ent), f"{tag}: the folded gradient of {h} was written by the chain + trunk call"
    _backward(model, spec, packed, out, d_out, stash, grads=grads, xyz=X, unfold=True, zero_folded=True, parts=L.BN_BWD_WGRAD_HEADS | L.BN_BWD_SKINNY)
    for k, v in first.items():
        if k.startswith("fc_net."):
            assert float(v.abs().max()) > 0 and torch.equal(v, grads[k]), f"{tag}: d {k} is not final after the chain + trunk call"
        else:
            assert float(v.abs().max()) == 0.0, f"{tag}: d {k} is not zero after the chain + trunk call (max {float(v.abs().max()):.3e})"
    TL._check_gradients(tag, dtype, _cpu64(grads), r["G64"], r["A1"], r["AK"], TL._n_extra(case, B, dtype))
    assert _fault_word() == 0


_PARTS_B = [c for c in RAW if c[1] == "B"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,sname,stride", _PARTS_B, ids=_ids(_PARTS_B))
def test_backward_in_parts_is_the_whole_backward_bitwise(name, sname, stride, dtype):
    """Property 8 on the generic set B (two point splits in the 16-bit modes), in the two-block ray form: the two part calls
    against BN_BWD_ALL (the reference of property 3), every parameter's gradient torch.equal.  The point split of a
    weight-gradient launch is taken from the launch's tile count (bn_wgrad_splits, csrc/field.h): with fewer jobs per launch
    the split count can only grow, and at these sizes the points per split stay at the floor (512 in the 16-bit modes, 256
    in fp32) either way, so the slabs and their fixed-order sums are the same."""
    from brdf_nerf_amd import _lib as L
    model, spec, cfg = _model(name, dtype)
    I = _inputs(name, sname, stride)
    d_out, want = _reference_grads(name, sname, stride, dtype, False)
    packed = model.repack(spec)
    out, stash, _ = _forward_set(model, spec, packed, dict(rays=I["rays"], z=I["z"]), dict(rays=I["rays"], z=I["z2"]), I["n1"], I["n_all"])
    grads = _zero_grads(model)
    _clear_folded(spec)
    pts = dict(rays=I["rays"], z=I["z"], z2=I["z2"])
    _backward(model, spec, packed, out, d_out, stash, grads=grads, unfold=False, zero_folded=False, parts=L.BN_BWD_CHAIN | L.BN_BWD_WGRAD_TRUNK, **pts)
    _backward(model, spec, packed, out, d_out, stash, grads=grads, unfold=True, zero_folded=True, parts=L.BN_BWD_WGRAD_HEADS | L.BN_BWD_SKINNY, **pts)
    _assert_same_grads(f"{name} {dtype} {sname} parts", grads, want, set(spec.used_param_names()))
    assert _fault_word() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,B", PS.LATTICE)
def test_lattice_points_as_one_sample_rays(name, B, dtype):
    """Property 9.  The lattice points as one-sample rays in two blocks over the same rays (point_set_cases.lattice_ray_blocks:
    ray r carries point r at z = 1 and point R + r at z2 = 2, exact; two blocks share their rays and the second launch starts
    at a tile multiple, so the set is the case's first 2 R points, R the tile multiple nearest B / 2): two ray-form forward
    launches, one two-block backward, held to the float64 reference of those 2 R points by the same forward and gradient
    checks (extra additions: 0)."""
    rb = PS.lattice_ray_blocks(name, B)
    n, R = rb["n"], rb["n"] // 2
    r, case, model, spec, packed = _lattice(name, n, dtype)
    rays, z, z2 = (rb[k].float().contiguous().to(DEV) for k in ("rays", "z", "z2"))
    out, stash, _ = _forward_set(model, spec, packed, dict(rays=rays, z=z), dict(rays=rays, z=z2), R, n)
    _check_lattice_out(f"{name} {dtype} {n} points as rays", r, out)
    G = _backward(model, spec, packed, out, case.coef[:n].float().contiguous().to(DEV), stash, rays=rays, z=z, z2=z2)
    TL._check_gradients(f"{name} {dtype} {n} points as rays", dtype, _cpu64(G), r["G64"], r["A1"], r["AK"], TL._n_extra(case, n, dtype))
    assert _fault_word() == 0
