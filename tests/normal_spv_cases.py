"""The rule of bn_normal_target_loss (include/brdfnerf_hip.h, "NormalLoss against per-ray target normals") in numpy float32, every
operation rounded on its own, and the inputs its tests share.  The statement is what the kernel is held to bit for bit; the
statement itself is held to the reference's NormalLoss(keyword='an') by tests/golden/normal_spv.npz."""
import numpy as np

F = np.float32


def statement(acc, ch, normals, valid_normal, valid_depth, lam, nonfinite=False):
    """-> dict: n_sel; term (R,) float32 per-ray loss terms (0 where nothing is added); grad (R, 3) float32 = what is ADDED to
    d_acc[:, ch:ch+3] (the update is d + grad in float32, so an entry of -0.0 / +0.0 matters to the bits: see apply());
    touched (R,) bool: rows the kernel writes; dropped (n_nan, n_inf): rays left out with `nonfinite`."""
    acc = np.asarray(acc, F)
    n_gt = np.asarray(normals, F)
    vn = np.asarray(valid_normal, F)
    vd = np.asarray(valid_depth, F)
    R = acc.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        sel = vd > 0                                            # NaN: False
        n_sel = int(sel.sum())
        term = np.zeros(R, F)
        grad = np.zeros((R, 3), F)
        touched = np.zeros(R, bool)
        if n_sel == 0:
            return dict(n_sel=0, term=term, grad=grad, touched=touched, dropped=(0, 0))
        k = F(lam) / (F(3.0) * F(n_sel))
        a = vn[:, None] * n_gt
        b = vn[:, None] * acc[:, ch:ch + 3]
        e = a - b
        ae = np.abs(e)
        t = k * ((ae[:, 0] + ae[:, 1]) + ae[:, 2])
        s = np.where(e > 0, F(-1.0), np.where(e < 0, F(1.0), F(0.0))).astype(F)
        gr = ((k * vn)[:, None] * s).astype(F)
        bad = ~(np.abs(t) <= F(3.0e38))
        drop = sel & bad if nonfinite else np.zeros(R, bool)
        keep = sel & ~drop
        term[keep] = t[keep]
        grad[keep] = gr[keep]
        touched[keep] = True
        dropped = (int((drop & np.isnan(t)).sum()), int((drop & ~np.isnan(t)).sum()))
    return dict(n_sel=n_sel, term=term, grad=grad, touched=touched, dropped=dropped)


def apply(d_acc, ray_loss, ch, st):
    """What the kernel leaves in d_acc / ray_loss given the statement `st`: float32 additions on the touched rows only."""
    d = np.array(d_acc, F, copy=True)
    rl = np.array(ray_loss, F, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = np.nonzero(st["touched"])[0]
        d[rows, ch:ch + 3] = d[rows, ch:ch + 3] + st["grad"][rows]
        rl[rows] = rl[rows] + st["term"][rows]
    return d, rl


def make_inputs(R, C, ch, seed, p_sel=0.6, p_vn=0.7):
    """Seeded inputs of one kernel case: acc (R,C), normals (R,3) unit, valid_normal, valid_depth in {0,1}, the d_acc and ray_loss
    the entry adds into."""
    g = np.random.default_rng(seed)
    acc = g.standard_normal((R, C)).astype(F)
    n = g.standard_normal((R, 3))
    n[:, 2] = np.abs(n[:, 2]) + 1.0
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    valid_normal = (g.random(R) < p_vn).astype(F)
    valid_depth = (g.random(R) < p_sel).astype(F)
    d_acc = g.standard_normal((R, C)).astype(F)
    ray_loss = g.random(R).astype(F)
    return dict(acc=acc, normals=normals, valid_normal=valid_normal, valid_depth=valid_depth, d_acc=d_acc, ray_loss=ray_loss)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def ulp_diff(a, b):
    """Largest distance in float32 units in the last place between two arrays of finite values of equal sign pattern (0 == bit-equal;
    +0 and -0 count as equal)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max()) if a.size else 0
