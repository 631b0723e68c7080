"""Semi-global aggregation of the altitude sweep's cost volume: what the scan kernel costs, and what it saves.  The volumes are
sweep_throughput.py's - altitude_sweep(want_cost=True) on the urban reliefs of 512 x 512 and 2048 x 2048 cells of 0.5 m under K = 3
images, Z = 17 / 65 offsets of 0.5 m - aggregated over 4 and 8 paths with p1 = 0.02, p2 = 0.16 (P1 = 256, P2 = 2048 quanta).

(a) by device events: bn_cost_paths alone, into a zeroed sum; its steps (cells x paths) per second and the bytes per second it must
    touch at least - (4 read + 4 read and 4 written by the atomic) x paths x Z H W;
(b) whole calls by a host clock, alternately in one process: aggregate_costs against what the parent commit offers for the same
    answer - the same recurrence in torch int32 operations on the device, vectorised over the lines of a direction and sequential
    along them (quanta and pick in torch as well); whether the two give equal level maps;
(c) with --resources (no GPU needed): VGPRs, scratch, LDS and waves per SIMD of the three kernels as the compiler reports them.
Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes profiles/aggregate_throughput.txt (or the path
given as the first argument; --resources appends to it).  Nothing here is a gate."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVELS, PATHS, STEP, K = (17, 65), (4, 8), 0.5, 3
P1_COST, P2_COST = 0.02, 0.16
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))
QINV = 1 << 20


def resources(out_path):
    from brdf_nerf_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        cmd = B.compile_command(os.path.join(B.CSRC, "aggregate.hip"), os.path.join(tmp, "aggregate.s"), asm=True)
        log = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    rows, got = [], None
    for l in log.splitlines():
        m = re.search(r"Function Name: \S*?(cost_quanta_kernel|cost_pick_kernel|cost_paths_kernelILi\d)", l)
        if m:
            got = {"name": m.group(1).replace("ILi", "<") + (">" if "ILi" in m.group(1) else "")}
            rows.append(got)
        for key, tag in (("VGPRs", " VGPRs:"), ("scratch", "ScratchSize [bytes/lane]:"), ("LDS", "LDS Size [bytes/block]:"),
                         ("waves", "Occupancy [waves/SIMD]:"), ("sgpr_spill", "SGPRs Spill:")):
            if got is not None and tag in l:
                got[key] = l.split(tag)[1].split()[0]
    with open(out_path, "a") as f:
        for got in rows:
            s = f"(c) {got['name']}: {got.get('VGPRs')} VGPRs, {got.get('scratch')} B of scratch per lane, {got.get('LDS')} B of LDS, " \
                f"{got.get('waves')} waves per SIMD, {got.get('sgpr_spill')} SGPRs held in VGPR lanes (gfx950, as the compiler reports them)"
            print(s)
            f.write(s + "\n")


def torch_aggregate(cost, quantum, P1, P2, mask):
    """The rule in torch on the device.  Every direction is sequential over rows (or, along the rows, over columns) and one int32
    expression over all lines and levels per step; a diagonal's predecessor is the neighbouring column of the previous row."""
    import torch
    c = cost.permute(1, 2, 0)
    known = ~torch.isnan(c)
    t = torch.where(known, c.double() / quantum, torch.zeros((), dtype=torch.float64, device=cost.device))
    q = torch.where(known, torch.round(t.clamp(0.0, QINV - 1.0)).to(torch.int32), torch.full((), QINV, dtype=torch.int32, device=cost.device))
    q = torch.where(known.any(-1, keepdim=True), q, torch.full((), -1, dtype=torch.int32, device=cost.device)).contiguous()
    cq = q.clamp(min=0)
    total = torch.zeros_like(cq)
    for b, (dj, di) in enumerate(DIRECTIONS):
        if not mask >> b & 1:
            continue
        along = cq.transpose(0, 1) if dj == 0 else cq                      # (steps, lines, Z)
        out = total.transpose(0, 1) if dj == 0 else total
        forward = dj > 0 or (dj == 0 and di > 0)
        shift = di if dj != 0 else 0
        n = along.shape[0]
        prev = None
        for s in (range(n) if forward else range(n - 1, -1, -1)):
            if prev is None:
                prev = along[s]
            else:
                m = prev.min(-1, keepdim=True).values
                msg = torch.minimum(prev, m + P2)
                msg[:, 1:] = torch.minimum(msg[:, 1:], prev[:, :-1] + P1)
                msg[:, :-1] = torch.minimum(msg[:, :-1], prev[:, 1:] + P1)
                msg -= m
                if shift:                                                      # the border column starts a line: no message
                    moved = torch.zeros_like(msg)
                    if shift > 0:
                        moved[1:] = msg[:-1]
                    else:
                        moved[:-1] = msg[1:]
                    msg = moved
                prev = along[s] + msg
            out[s] += prev
    valid = (q >= 0) & (q < QINV)
    key = torch.where(valid, total, torch.full((), 2 ** 31 - 1, dtype=torch.int32, device=cost.device))
    low = key.min(-1, keepdim=True).values
    Z = key.shape[-1]
    first = torch.where(key == low, torch.arange(Z, device=cost.device), torch.full((), Z, device=cost.device)).min(-1).values
    return torch.where(valid.any(-1), first, torch.full_like(first, -1)).to(torch.int32)


def measure():
    import numpy as np
    import torch
    import orthophoto_cases as O
    from dsm_throughput import device_ms, say
    from mosaic_throughput import cameras
    from orthophoto_throughput import IMAGE, RES, ZONE
    from sweep_throughput import alternately
    from visibility_throughput import urban
    from brdf_nerf_amd import Grid, Rpc, aggregate_costs, altitude_sweep, camera
    from brdf_nerf_amd import functions as Fn
    dev = torch.device("cuda", 0)
    say(f"urban relief, 0.5 m cells, zone {ZONE} north; the cost volumes of altitude_sweep under K = {K} images of {IMAGE} x {IMAGE} x 3 and "
        f"offsets of {STEP} m; p1 = {P1_COST}, p2 = {P2_COST}, quantum p1 / 256; device {torch.cuda.get_device_name(0)}")
    torch.manual_seed(0)
    images = [torch.rand((IMAGE * IMAGE, 3), device=dev) for _ in range(K)]
    quantum = P1_COST / 256.0
    with torch.no_grad():
        for side in (512, 2048):
            relief = urban(side)
            xoff, yoff = O.site_grid("z17", side, side, RES)
            grid = Grid(xoff, yoff, RES, side, side)
            dsm = torch.from_numpy(relief).to(dev)
            lo_alt, hi_alt = float(np.nanmin(relief)), float(np.nanmax(relief))
            rpcs = [Rpc.from_dict(d) for d in cameras(K)]
            dirs = torch.stack([torch.as_tensor(camera.view_direction(r, ZONE, False, lo_alt, hi_alt, device=dev)) for r in rpcs])
            views = [(images[k], IMAGE, IMAGE, rpcs[k]) for k in range(K)]
            for Z in LEVELS:
                offsets = (np.arange(Z) - Z // 2) * STEP
                cost = altitude_sweep(views, dsm, grid, ZONE, offsets, view_dirs=dirs, want_cost=True)["cost"]
                quanta, counters = Fn.cost_quanta(cost, quantum)
                say(f"{side} x {side}, Z = {Z}: cells with a result, valid pairs, capped pairs {counters.tolist()}")
                total = torch.empty_like(quanta)
                for paths in PATHS:
                    mask = 0x0F if paths == 4 else 0xFF

                    def scan():
                        total.zero_()
                        Fn.cost_paths(quanta, 256, 2048, mask, total)
                    lo, med = device_ms(scan, 5)
                    zero, _ = device_ms(total.zero_, 5)
                    lo, med = lo - zero, med - zero
                    steps, moved = side * side * paths, 12 * paths * Z * side * side
                    say(f"(a) {side} x {side}, Z = {Z}, {paths} paths: bn_cost_paths {lo:.3f} ms (median {med:.3f}; the zeroing of sum, {zero:.3f} ms, "
                        f"taken off) = {steps / lo / 1e6:.2f} G steps/s, {moved / lo / 1e9:.3f} TB/s of the {moved / 1e9:.2f} GB it must touch")
                    got = {}

                    def fused():
                        got["ours"] = aggregate_costs(cost, P1_COST, P2_COST, paths=paths)["level"]

                    def composed():
                        got["torch"] = torch_aggregate(cost, quantum, 256, 2048, mask)
                    (t, t_med), (bt, bt_med) = alternately(fused, composed, 2)
                    same = torch.equal(got["ours"], got["torch"])
                    say(f"(b) {side} x {side}, Z = {Z}, {paths} paths: aggregate_costs, whole call {t * 1e3:.2f} ms (median {t_med * 1e3:.2f}); the "
                        f"recurrence in torch int32 operations {bt * 1e3:.2f} ms (median {bt_med * 1e3:.2f}): {bt / t:.1f} times; level maps "
                        f"{'EQUAL' if same else 'DIFFER'}")
                    del got
                del cost, quanta, total
                torch.cuda.empty_cache()
    del images
    torch.cuda.empty_cache()
    try:
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        line = [json.loads(s) for s in run.stdout.splitlines() if s.startswith("{")][-1]
        say(f"# box-speed indicator: bench.py in the same visit, same box: {line['value'] / 1e3:.1f} k train rays/s, {line['ms_per_step']:.3f} ms "
            f"per step (BASELINE config 2, bf16).")
    except Exception as e:      # the indicator is a note, not a measurement of this file
        say(f"# box-speed indicator: bench.py did not give a result line ({type(e).__name__})")


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "aggregate_throughput.txt")
    if "--resources" in sys.argv:
        return resources(out_path)
    from dsm_throughput import LINES
    try:
        measure()
    finally:
        with open(out_path, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
