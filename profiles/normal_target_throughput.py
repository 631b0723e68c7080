"""NormalLoss against the rays' target normals (bn_normal_target_loss, --nr_spv_type 3): the two launches of the entry at R = 4096
and 65,536 on buffers made once, by device events (60 % of the rays selected, C = 16); and the launch-lean step of an RPV model
with analytic normals at R = 4096, S = G = 64, bf16 - replayed from its HIP graph - with and without the term, by device events
over the replay.  Ends with bench.py in a child process as the box-speed indicator of the visit.  Writes
profiles/normal_target_throughput.txt (or the path given as the first argument).  Nothing here is a gate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from dsm_throughput import LINES, device_ms, say  # noqa: E402
from brdf_nerf_amd import functions as Fn  # noqa: E402


def launches(R, dev, C=16, ch=7):
    g = torch.Generator(device=dev).manual_seed(R)
    acc = torch.randn(R, C, device=dev, generator=g)
    d_acc = torch.zeros(R, C, device=dev)
    n = torch.randn(R, 3, device=dev, generator=g)
    normals = n / n.norm(dim=-1, keepdim=True)
    vn = (torch.rand(R, device=dev, generator=g) < 0.8).float()
    vd = (torch.rand(R, device=dev, generator=g) < 0.6).float()
    ray_loss = torch.zeros(R, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    nf = torch.zeros(2, dtype=torch.int64, device=dev)
    lo, med = device_ms(lambda: Fn.normal_target_loss(acc, ch, normals, vn, vd, 0.1, d_acc, ray_loss=ray_loss, nonfinite=nf, count=count), 50)
    say(f"bn_normal_target_loss R = {R}, C = {C}: count + per-ray launch {lo * 1e3:.1f} us (median {med * 1e3:.1f}); n_sel {int(count.item())}")


def lean_step(dev, lam):
    from oracle.config import FieldConfig
    from test_gpu_parity import build_model, make_args
    from brdf_nerf_amd.raytable import synthetic_table
    from brdf_nerf_amd.trainer import FusedTrainer
    cfg = FieldConfig(feat=256, n_samples=64, guided_samples=64, funcM=1, funcF=1, funcH=1, normal="analystic")
    args = make_args(cfg, "bf16")
    torch.manual_seed(0)
    tr = FusedTrainer(build_model(cfg, 5, "bf16"), args, lr=5e-4, ds_lambda=10.0, strict_rng=False, nr_spv_lambda=lam, nr_spv_type=3)
    tr.graph_after = 1
    b = synthetic_table(4096, device=dev, seed=2, with_normals=True).next_batch(4096)
    step = lambda: tr.step(b["rays"], b["rgbs"], valid_depth=b["valid_depth"], depths=b["depths"], depth_std=b["depth_std"],
                           apply_brdf=True, apply_theta=True, cos_irra_on=True, near_far=(0.0, 2.0), normals=b["normals"],
                           valid_normal=b["valid_normal"])
    for _ in range(4):
        step()
    lo, med = device_ms(step, 30)
    assert len(tr._graphs) == 1
    return lo, med


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "normal_target_throughput.txt")
    dev = torch.device("cuda", 0)
    say(f"device {torch.cuda.get_device_name(0)}; normal_target_count_kernel: one workgroup of 1024; normal_target_ray_kernel: a lane per "
        f"ray, blocks of 256")
    for R in (4096, 65536):
        launches(R, dev)
    for rnd in range(2):          # alternately: the box is shared
        off = lean_step(dev, 0.0)
        on = lean_step(dev, 0.1)
        say(f"lean step (RPV, analytic normals, feat 256, R = 4096, S = G = 64, bf16, graph replay) round {rnd}: without the term "
            f"{off[0]:.3f} ms (median {off[1]:.3f}), with it {on[0]:.3f} ms (median {on[1]:.3f})")
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
