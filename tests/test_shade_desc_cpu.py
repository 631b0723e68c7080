"""The descriptor checks of the six entry points that shade with a bn_shade_desc (csrc/shade_row.h shade_desc_check and the
clauses each entry keeps): a descriptor with ONE fault is refused by every entry under the entry's own name with the clause that
names the fault - or is taken, where the entry has nothing against it.  No kernel is needed: a refusal comes before any launch.
Every buffer is still a real allocation of the right size (R = 2, S = G = 3, K = 1; on the device where there is one), so a
refusal that got lost would launch a valid tiny kernel and show as a wrong status, never as a walk over dummy addresses.

EXPECT was recorded once from the library of the commit before the checks were folded into one function and is not computed.
A clause is a piece of that library's message.  Where bn_sample_brdf_* took the wording of the other entries then (their
messages were worded apart: "C=3, row stride ..." for "C=3 unsupported", one "normal channel" clause for the range and for the
missing field), it is the piece both wordings share."""
import ctypes as C

import pytest
import torch

from brdf_nerf_amd import _lib as L

R, S, G, K = 2, 3, 3, 1
BN_MAX_CH = 32                       # csrc/common.h
BN_EINVAL, BN_ELAUNCH = -1, -3       # include/brdfnerf_hip.h bn_status
CMAX = BN_MAX_CH + 1                 # every buffer holds rows of the widest descriptor of the table
ENTRIES = ("ray_shade_loss", "sample_brdf_forward", "sample_brdf_backward", "ray_shade_dirs", "sample_shade_dirs", "sun_shade_dirs")


def desc(kind=L.BN_SHADE_RPV, C_=16, ch_normal=4, ch_p0=7, ch_p1=10, ch_p2=13, shell=0):
    """A valid descriptor (RPV with its three heads, unless told otherwise)."""
    d = L.ShadeDesc()
    d.kind, d.C, d.ch_normal, d.ch_p0, d.ch_p1, d.ch_p2, d.shell = kind, C_, ch_normal, ch_p0, ch_p1, ch_p2, shell
    d.hpk_scl, d.f0, d.rgb_padding, d.lambda_rgb = 1.0, 0.04, 0.001, 1.0
    return d


def hapke(**kw):
    return desc(kind=L.BN_SHADE_HAPKE, **kw)


# name -> (descriptor, directions given)
FAULTS = {
    "C=3": (desc(C_=3), True),
    "C=MAX+1": (desc(C_=BN_MAX_CH + 1), True),
    "kind=4": (desc(kind=4), True),
    "kind=-1": (desc(kind=-1), True),
    "ch_normal=2": (desc(ch_normal=2), True),
    "ch_normal=C-2": (desc(ch_normal=14), True),
    "brdf_without_normal": (desc(ch_normal=-1), True),
    "brdf_without_dirs": (desc(), False),
    "wide_head_at_C-1": (desc(ch_p1=15), True),
    "hapke_theta_at_C-1": (hapke(ch_p2=15), True),          # one channel wide: in range
    "microfacet_without_roughness": (desc(kind=L.BN_SHADE_MICROFACET, ch_p0=-1, ch_p1=-1, ch_p2=-1), True),
    "hapke_no_b_shell=0": (hapke(ch_p0=-1, shell=0), True),
    "hapke_no_b_shell=4": (hapke(ch_p0=-1, shell=4), True),
}

# fault -> the clause of every entry, or one clause per entry in the order of ENTRIES; None: the entry takes the descriptor
_FIELD = "BRDF shading needs a normal field and the ray"     # "... ray directions" / "... ray or view directions" then
EXPECT = {
    "C=3": ("C=3 unsupported", "C=3", "C=3", "C=3 unsupported", "C=3 unsupported", "C=3 unsupported"),
    "C=MAX+1": ("C=33 unsupported", "C=33", "C=33", "C=33 unsupported", "C=33 unsupported", "C=33 unsupported"),
    "kind=4": ("kind=4", "kind=4", "kind=4", "kind=4", "kind=4 (a Lambertian colour is a function of the composited sums", "kind=4"),
    "kind=-1": ("kind=-1", "kind=-1", "kind=-1", "kind=-1", "kind=-1 (a Lambertian colour is a function of the composited sums", "kind=-1"),
    "ch_normal=2": "normal channel 2 outside [4, 16)",
    "ch_normal=C-2": "normal channel 14 outside [4, 16)",
    "brdf_without_normal": (_FIELD, "normal", "normal", _FIELD, _FIELD, _FIELD),      # then: "normal channel -1 outside [4, 16)"
    "brdf_without_dirs": (_FIELD, "null argument", "null argument", _FIELD, _FIELD, _FIELD),
    "wide_head_at_C-1": ("parameter channels (7, 15, 13) outside [4, 16)", "parameter channels", "parameter channels",
                         "parameter channels (7, 15, 13) outside [4, 16)", "parameter channels (7, 15, 13) outside [4, 16)",
                         "parameter channels (7, 15, 13) outside [4, 16)"),
    "hapke_theta_at_C-1": None,
    "microfacet_without_roughness": "microfacet needs the roughness channel",
    "hapke_no_b_shell=0": "Hapke without b needs shell_hapke in {1,2,3}",
    "hapke_no_b_shell=4": "Hapke without b needs shell_hapke in {1,2,3}",
}


def _buf(n):
    """n floats -> (owner, pointer): a device tensor where there is a device, else host memory."""
    if torch.cuda.is_available():
        t = torch.full((n,), 0.5, dtype=torch.float32, device="cuda")
        return t, C.c_void_p(t.data_ptr())
    a = (C.c_float * n)(*([0.5] * n))
    return a, C.cast(a, C.c_void_p)


def call(entry, d, dirs):
    """-> (status, message) of one entry point for descriptor d, every other argument valid."""
    lib = L.lib()
    keep = []

    def buf(n):
        o, p = _buf(n)
        keep.append(o)
        return p
    N = R * S
    rays_d = buf(R * 3) if dirs else None
    dp = C.byref(d)
    if entry == "ray_shade_loss":
        st = lib.bn_ray_shade_loss(dp, buf(R * CMAX), buf(R), buf(R), None, rays_d, 3, None, 0, buf(R * 3), None, 0, None, 0, None, 0, None, 0,
                                   R, None, None, None, 0, buf(R * CMAX), buf(R), buf(R), None, None, None)
    elif entry in ("sample_brdf_forward", "sample_brdf_backward"):
        rays = buf(R * 11) if dirs else None
        fn = getattr(lib, "bn_" + entry)
        tail = (buf(N * 4), 4, None) if entry.endswith("forward") else (buf(N * 4), 4, buf(N * CMAX), None)
        st = fn(dp, buf(N * CMAX), rays, R, 11, 8, N, N, S, 0, *tail)
    elif entry == "ray_shade_dirs":
        st = lib.bn_ray_shade_dirs(dp, buf(R * CMAX), buf(R), rays_d, 3, buf(K * 3), None, R, K, buf(K * R * 3), None, None)
    elif entry == "sample_shade_dirs":
        st = lib.bn_sample_shade_dirs(dp, buf(N * CMAX), buf(N), rays_d, 3, buf(K * 3), None, R, S, K, buf(K * R * 3), 3 * R, None, 0, None)
    else:
        st = lib.bn_sun_shade_dirs(dp, buf(K * R * G), buf(K * R * G), None, 0.0, buf(R * CMAX), buf(R), None, None, rays_d, 3, buf(K * 3),
                                   R, G, K, buf(K * R * 3), 3 * R, None, 0, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return st, lib.bn_last_error().decode()


def test_the_table_is_complete():
    assert set(EXPECT) == set(FAULTS)
    assert all(isinstance(v, (str, type(None))) or len(v) == len(ENTRIES) for v in EXPECT.values())


def test_a_valid_descriptor_is_taken_by_every_entry():
    for kind_desc in (desc(), hapke(), desc(kind=L.BN_SHADE_MICROFACET, ch_p1=-1, ch_p2=-1)):
        for entry in ENTRIES:
            st, msg = call(entry, kind_desc, True)
            assert st == 0 if torch.cuda.is_available() else st in (0, BN_ELAUNCH), (entry, st, msg)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_single_fault_descriptor(fault):
    d, dirs = FAULTS[fault]
    want = EXPECT[fault]
    for i, entry in enumerate(ENTRIES):
        clause = want if isinstance(want, (str, type(None))) else want[i]
        st, msg = call(entry, d, dirs)
        if clause is None:
            # taken: the tiny launch runs - or, without a device, fails as a launch, not as an argument
            assert st == 0 if torch.cuda.is_available() else st in (0, BN_ELAUNCH), (entry, st, msg)
        else:
            assert st == BN_EINVAL and msg.startswith(entry + ":") and clause in msg, (entry, st, msg, clause)
