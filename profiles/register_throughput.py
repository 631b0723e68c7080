"""Registration throughput: (a) register_xy on a 512 x 512 pair (four levels: 512, 256, 128, 64) and each launch alone -
bn_grid_halve, bn_ncc_moments at r = 5 per level, bn_dsm_shift_diff; (b) the same on a 1024 x 1024 pair; (c) the same search as
float64 torch ops on the device, one shift at a time (the masked Pearson correlation of two slices), for comparison; (d)
score_view(register='xy') against register='z' on the configuration of profiles/metrics_throughput.py.  Kernel times by device
events, whole calls by a host clock around a synchronise (register_xy reads the moments back once per level, so its time holds
those copies and the host-side argmax).  Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes
profiles/register_throughput.txt (or the path given as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import torch  # noqa: E402
import bench  # noqa: E402
from dsm_throughput import LINES, device_ms, say, timed  # noqa: E402
from brdf_nerf_amd import SceneFrame, apply_registration, dsm_image, load_model, register_xy, score_view  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402


def pair(H, W, shift, offset, gen, dev):
    """A smooth surface with steps and 0.05 m noise; the prediction is the ground truth moved by `shift` cells, lowered by
    `offset`, with noise of its own and 5 % NaN cells."""
    m = 32
    jj, ii = torch.meshgrid(torch.arange(H + 2 * m, dtype=torch.float64), torch.arange(W + 2 * m, dtype=torch.float64), indexing="ij")
    f = 40.0 + 4.0 * torch.sin(jj / 17.0) * torch.cos(ii / 23.0) + 0.02 * ii
    for _ in range(40):
        r0, c0 = int(torch.randint(0, H, (1,), generator=gen)), int(torch.randint(0, W, (1,), generator=gen))
        f[r0:r0 + 30, c0:c0 + 40] += float(torch.rand(1, generator=gen)) * 12.0 + 3.0
    dx, dy = shift
    gt = f[m:m + H, m:m + W] + 0.05 * torch.randn(H, W, generator=gen, dtype=torch.float64)
    pred = f[m - dy:m - dy + H, m - dx:m - dx + W] - offset + 0.05 * torch.randn(H, W, generator=gen, dtype=torch.float64)
    pred[torch.rand(H, W, generator=gen) < 0.05] = float("nan")
    return pred.float().to(dev), gt.float().to(dev)


def torch_corr(u, v, dx, dy):
    """The correlation of one shift in float64 torch ops: the slices that overlap, the pairs where both are finite."""
    H, W = u.shape
    j0, j1, i0, i1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    a, b = u[j0:j1, i0:i1], v[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    ok = torch.isfinite(a) & torch.isfinite(b)
    n = ok.sum()
    a, b = torch.where(ok, a, 0.0), torch.where(ok, b, 0.0)
    ma, mb = a.sum() / n, b.sum() / n
    da, db = torch.where(ok, a - ma, 0.0), torch.where(ok, b - mb, 0.0)
    return (da * db).sum() / torch.sqrt((da * da).sum() * (db * db).sum())


def torch_level(u, v, dx0, dy0, r):
    c = torch.stack([torch_corr(u, v, dx, dy) for dy in range(dy0 - r, dy0 + r + 1) for dx in range(dx0 - r, dx0 + r + 1)])
    at = int(torch.argmax(torch.nan_to_num(c, nan=-2.0)))
    return dx0 - r + at % (2 * r + 1), dy0 - r + at // (2 * r + 1)


def torch_register(pred, gt, r=5, min_size=100):
    pyr = [(gt.double(), pred.double())]
    while min(pyr[-1][0].shape) > min_size:
        pyr.append((Fn.grid_halve(pyr[-1][0]), Fn.grid_halve(pyr[-1][1])))       # the pyramid is not what is compared
    dx = dy = 0
    for u, v in reversed(pyr):
        dx, dy = torch_level(u, v, 2 * dx, 2 * dy, r)
    return dx, dy


def one_size(H, W, shift, gen, dev, tag):
    pred, gt = pair(H, W, shift, 3.25, gen, dev)
    reg = register_xy(pred, gt)
    t_reg, t_reg_med = timed(lambda: register_xy(pred, gt), 5)
    say(f"({tag}) {H} x {W}, true shift {shift}: register_xy -> {reg['levels']}, b {reg['b']:.6f}, k {reg['k']}: {t_reg * 1e3:.3f} ms "
        f"(median {t_reg_med * 1e3:.3f}) with {len(reg['levels'])} device-to-host copies of 121 x 6 int64")
    u, v = gt.double().contiguous(), pred.double().contiguous()
    level = 0
    while True:
        sums = torch.zeros((121, 6), dtype=torch.int64, device=dev)
        skipped = torch.zeros(1, dtype=torch.int64, device=dev)
        Hl, Wl, dxl, dyl = reg["levels"][len(reg["levels"]) - 1 - level]
        m_ms, m_med = device_ms(lambda: Fn.ncc_moments(u, v, reg["pivot"], reg["k"], dxl, dyl, 5, sums=sums, skipped=skipped))
        pairs = 121 * Hl * Wl
        line = f"    level {level} ({Hl} x {Wl}): bn_ncc_moments r = 5 {m_ms:.3f} ms (median {m_med:.3f}) = {pairs / m_ms / 1e6:.1f} G pairs/s"
        if min(Hl, Wl) <= 100:
            say(line)
            break
        h_ms, h_med = device_ms(lambda: Fn.grid_halve(u))
        say(line + f"; bn_grid_halve {h_ms:.3f} ms (median {h_med:.3f})")
        u, v, level = Fn.grid_halve(u), Fn.grid_halve(v), level + 1
    s_ms, s_med = device_ms(lambda: Fn.dsm_shift_diff(pred, gt, reg["dx"], reg["dy"], reg["b"]))
    out = apply_registration(pred, gt, reg["dx"], reg["dy"], reg["b"])
    say(f"    bn_dsm_shift_diff {s_ms:.3f} ms (median {s_med:.3f}); mae after registration {out['mae']:.6f} m")
    return pred, gt, reg, t_reg


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "register_throughput.txt")
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    say(f"device {torch.cuda.get_device_name(0)}; moments: one integer atomic per (shift, moment) per block, row groups combined in LDS")
    pred, gt, reg, t_reg = one_size(512, 512, (16, -8), gen, dev, "a")
    one_size(1024, 1024, (24, -16), gen, dev, "b")
    t_t, t_t_med = timed(lambda: torch_register(pred, gt), 2)
    say(f"(c) 512 x 512: the same search in float64 torch ops, one shift at a time (4 x 121 correlations): {t_t * 1e3:.1f} ms (median "
        f"{t_t_med * 1e3:.1f}) -> {torch_register(pred, gt)} against {(reg['dx'], reg['dy'])}; {t_t / t_reg:.1f} x register_xy")

    H = W = 512
    N, chunk, config, dtype = H * W, 16384, "rpv_nan", "bf16"
    rays = bench.synthetic_batch(N, 3, dev)["rays"]
    args = bench.make_args(4096, 64, 64, dtype, **bench.CONFIG_FLAGS[config][0])
    torch.manual_seed(0)
    models = {"coarse": load_model(args).to(dev)}
    flags = dict(bench.CONFIG_FLAGS[config][1])
    rgbs = torch.rand(N, 3, generator=gen).to(dev)
    frame = SceneFrame((368412.25, 3359871.75, 12.5), 128.0)
    with torch.no_grad():
        first = dsm_image(models, args, rays, frame, chunk=chunk, **flags)
        grid = first["grid"]
        gt_dsm = torch.roll(torch.nan_to_num(first["dsm"], nan=12.5), (2, -2), (0, 1)) + 0.3
        kw = dict(frame=frame, gt_dsm=gt_dsm, grid=grid, chunk=chunk, **flags)
        t_z, t_z_med = timed(lambda: score_view(models, args, rays, rgbs, H, W, register="z", **kw), 3)
        t_xy, t_xy_med = timed(lambda: score_view(models, args, rays, rgbs, H, W, register="xy", **kw), 3)
        z = score_view(models, args, rays, rgbs, H, W, register="z", **kw)
        xy = score_view(models, args, rays, rgbs, H, W, register="xy", **kw)
    say(f"(d) {config} {dtype}, S = G = 64, chunk {chunk}; DSM grid {grid.width} x {grid.height}: score_view register='z' {t_z * 1e3:.1f} ms "
        f"(median {t_z_med * 1e3:.1f}), register='xy' {t_xy * 1e3:.1f} ms (median {t_xy_med * 1e3:.1f}) -> {(t_xy - t_z) * 1e3:+.1f} ms")
    say(f"    z: mae {z['mae']:.4f} mae_nr {z['mae_nr']:.4f} shift {z['shift']:.4f}; xy: mae {xy['mae']:.4f} mae_nr {xy['mae_nr']:.4f} shift "
        f"{xy['shift']:.4f} (dx, dy) ({xy['dx']}, {xy['dy']})")
    del models
    torch.cuda.empty_cache()
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        line = [json.loads(s) for s in run.stdout.splitlines() if s.startswith("{")][-1]
        say(f"# box-speed indicator: bench.py in the same visit, same box: {line['value'] / 1e3:.1f} k train rays/s, {line['ms_per_step']:.3f} ms "
            f"per step (BASELINE config 2, bf16).")
    except Exception as e:      # the indicator is a note, not a measurement of this file
        say(f"# box-speed indicator: bench.py did not give a result line ({type(e).__name__})")
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
