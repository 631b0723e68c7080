"""torch.autograd.Function wrappers over the C ABI (include/brdfnerf_hip.h).

PyTorch is plumbing here: it owns device memory and the stream and stitches the autograd graph;
every numerical step of the hot path runs in the HIP library.  No CPU fallback exists.
"""
import ctypes as C
import math
import numbers
import os

import torch

from . import _lib as L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "C ABI needs contiguous device tensors"
    return C.c_void_p(t.data_ptr())


def _f32(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


# ----------------------------------------------------------------------------------------- field MLP
class FieldSpec:
    """Host-side description of one evaluation of the field: which heads, which dtype."""

    def __init__(self, feat, layers, skip, pe_freqs, act, dtype, heads, normal_lr, normal_an=False, fold_feats=None,
                 dir_dim=0, dir_freqs=0, t_dim=0):
        # heads: list of (name, n_out, kind); heads[0] must be ("rgb_from_xyzdir", 3, PLAIN)
        self.feat, self.layers, self.skip, self.pe_freqs, self.act, self.dtype = feat, layers, skip, pe_freqs, act, dtype
        self.heads, self.normal_lr, self.normal_an = list(heads), bool(normal_lr), bool(normal_an)
        # feats_from_xyz is linear and feeds only the heads' first (linear) layers: W1 (Wf y + bf) + b1 = (W1 Wf) y + (W1 bf + b1).
        # Folding the two (one small GEMM per head per weight update, fold()) removes an F x F product per point from the
        # forward, the backward chain and the weight-gradient kernels; unfold_grads() takes the folded gradients back to
        # W1, b1, Wf, bf by the chain rule.  BRDFNERF_FOLD_FEATS=0 keeps the layer-by-layer evaluation.
        if fold_feats is None:
            fold_feats = os.environ.get("BRDFNERF_FOLD_FEATS", "1") != "0"
        self.fold_feats = bool(fold_feats)
        # --input_viewdir: the rgb head's first layer also reads the (encoded) view direction, dir_dim extra input columns
        self.dir_dim, self.dir_freqs = int(dir_dim), int(dir_freqs)
        if self.dir_dim and not self.fold_feats:
            raise NotImplementedError("--input_viewdir needs the folded feats layer (BRDFNERF_FOLD_FEATS=1, the default)")
        # --beta: head 1 (kind BN_HEAD_BETA) also reads the per-image embedding, t_dim extra input columns
        self.t_dim = int(t_dim)
        if (self.t_dim > 0) != (len(self.heads) > 1 and self.heads[1][2] == L.BN_HEAD_BETA):
            raise ValueError("t_dim goes with a beta head at index 1")
        if self.t_dim and not self.fold_feats:
            raise NotImplementedError("--beta needs the folded feats layer (BRDFNERF_FOLD_FEATS=1, the default)")
        self.folded, self.fold_grads = {}, {}
        d = L.FieldDesc()
        d.feat, d.layers, d.skip, d.pe_freqs, d.act, d.dtype = feat, layers, skip, pe_freqs, act, dtype
        d.fold_feats = int(self.fold_feats)
        d.dir_dim, d.dir_freqs, d.t_dim = self.dir_dim, self.dir_freqs, self.t_dim
        d.n_heads = len(self.heads)
        c0 = 5 if self.t_dim else 4                     # [rgb3, sigma, (beta)]
        c = c0 + (3 if normal_an else 0) + (3 if normal_lr else 0)
        self.head_cols = []
        for i, (_, n_out, kind) in enumerate(self.heads):
            d.head_out[i], d.head_kind[i] = n_out, kind
            if i == 0:
                self.head_cols.append((0, 3))
            elif kind == L.BN_HEAD_BETA:
                self.head_cols.append((4, 1))
            else:
                w = n_out if kind in (L.BN_HEAD_PLAIN, L.BN_HEAD_HAPKE_THETA) else 3
                self.head_cols.append((c, w))
                c += w
        d.normal_lr, d.normal_an, d.out_channels = int(normal_lr), int(normal_an), c
        self.desc, self.out_channels = d, c
        self.ch_beta = 4 if self.t_dim else -1
        self.ch_normal_an = c0 if normal_an else -1
        self.ch_normal_lr = (c0 + 3 if normal_an else c0) if normal_lr else -1
        self.packed_bytes = L.lib().bn_field_packed_bytes(C.byref(d))
        if self.packed_bytes == 0:
            raise RuntimeError("bn_field_packed_bytes: " + L.lib().bn_last_error().decode())

    def key(self):
        return (self.feat, self.layers, self.skip, self.pe_freqs, self.act, self.dtype, tuple(self.heads), self.normal_lr,
                self.normal_an, self.fold_feats, self.dir_dim, self.dir_freqs, self.t_dim)

    def params_struct(self, named, grads=False):
        """named: dict state_dict-key -> tensor (parameters, or same-shaped gradient buffers)."""
        s = L.FieldGrads() if grads else L.FieldParams()
        for l in range(self.layers):
            s.trunk_w[l] = named[f"fc_net.{2*l}.weight"].data_ptr()
            s.trunk_b[l] = named[f"fc_net.{2*l}.bias"].data_ptr()
        s.sigma_w, s.sigma_b = named["sigma_from_xyz.0.weight"].data_ptr(), named["sigma_from_xyz.0.bias"].data_ptr()
        s.feats_w, s.feats_b = named["feats_from_xyz.weight"].data_ptr(), named["feats_from_xyz.bias"].data_ptr()
        for i, (name, _, _) in enumerate(self.heads):
            s.head_w1[i], s.head_b1[i] = named[f"{name}.0.weight"].data_ptr(), named[f"{name}.0.bias"].data_ptr()
            s.head_w2[i], s.head_b2[i] = named[f"{name}.2.weight"].data_ptr(), named[f"{name}.2.bias"].data_ptr()
        if self.fold_feats:
            if grads:        # the library accumulates d/d(folded w1, b1) here; feats_* are produced by unfold_grads()
                s.feats_w = s.feats_b = None
                for i, (name, _, _) in enumerate(self.heads):
                    w1 = named[f"{name}.0.weight"]
                    ent = self.fold_grads.get(name)
                    if ent is None or ent[0].device != w1.device:
                        ent = (torch.zeros(w1.shape[0], self.feat, dtype=torch.float32, device=w1.device),
                               torch.zeros(w1.shape[0], dtype=torch.float32, device=w1.device))
                        self.fold_grads[name] = ent
                    s.head_w1[i], s.head_b1[i] = ent[0].data_ptr(), ent[1].data_ptr()
            else:
                if any(name not in self.folded for name, _, _ in self.heads):
                    self.fold(named)     # a spec evaluated with another spec's packed weights (sigma-only passes)
                for i, (name, _, _) in enumerate(self.heads):
                    s.head_w1[i], s.head_b1[i] = self.folded[name][0].data_ptr(), self.folded[name][1].data_ptr()
        if self.normal_lr:
            s.normal_w, s.normal_b = named["grad_from_xyz.weight"].data_ptr(), named["grad_from_xyz.bias"].data_ptr()
        if self.dir_dim:        # direction columns of the rgb head's first layer (parameters, or their gradient buffer)
            w = named[f"{self.heads[0][0]}.0.weight"]
            assert w.shape[1] == self.feat + self.dir_dim and w.is_contiguous()
            s.head0_wdir, s.head0_wdir_ld = w.data_ptr() + 4 * self.feat, w.shape[1]
        if self.t_dim:          # embedding columns of the beta head's first layer
            w = named[f"{self.heads[1][0]}.0.weight"]
            assert w.shape[1] == self.feat + self.t_dim and w.is_contiguous()
            s.head1_wt, s.head1_wt_ld = w.data_ptr() + 4 * self.feat, w.shape[1]
        return s

    def _fold_desc(self, named, named_grads=None, with_accumulators=True):
        """bn_fold_desc over this spec's heads (functions.fold / unfold_grads)."""
        d = L.FoldDesc()
        wf, bf = named["feats_from_xyz.weight"], named["feats_from_xyz.bias"]
        assert wf.is_contiguous() and wf.dtype == torch.float32
        d.n_heads, d.F = len(self.heads), self.feat
        d.wf, d.bf = wf.data_ptr(), bf.data_ptr()
        keep = [wf, bf]
        for i, (name, _, _) in enumerate(self.heads):
            w1, b1 = named[f"{name}.0.weight"], named[f"{name}.0.bias"]
            assert w1.is_contiguous() and w1.dtype == torch.float32
            d.rows = w1.shape[0]
            d.w1[i], d.w1_ld[i], d.b1[i] = w1.data_ptr(), w1.shape[1], b1.data_ptr()
            ent = self.folded.get(name)
            if ent is None or ent[0].device != w1.device:
                ent = (torch.empty(w1.shape[0], self.feat, dtype=torch.float32, device=w1.device), torch.empty_like(b1))
                self.folded[name] = ent
            d.w_fold[i], d.b_fold[i] = ent[0].data_ptr(), ent[1].data_ptr()
            acc = self.fold_grads.get(name) if with_accumulators else None
            d.m[i], d.s[i] = (acc[0].data_ptr(), acc[1].data_ptr()) if acc is not None else (None, None)
            if named_grads is not None:
                dw1, db1 = named_grads[f"{name}.0.weight"], named_grads[f"{name}.0.bias"]
                assert dw1.stride(-1) == 1
                d.d_w1[i], d.d_w1_ld[i], d.d_b1[i] = dw1.data_ptr(), dw1.stride(0), db1.data_ptr()
        if named_grads is not None:
            d.d_wf, d.d_bf = named_grads["feats_from_xyz.weight"].data_ptr(), named_grads["feats_from_xyz.bias"].data_ptr()
        return d, keep

    @torch.no_grad()
    def fold(self, named):
        """(W1 Wf, W1 bf + b1) per head, refreshed whenever the weights are re-packed (bn_fold_heads: one launch; it also
        clears the folded-gradient accumulators, which the weight-gradient kernels add to)."""
        named = {k: v.detach() for k, v in named.items()}
        d, _keep = self._fold_desc(named)
        L.check(L.lib().bn_fold_heads(C.byref(d), _stream()), "bn_fold_heads")

    @torch.no_grad()
    def unfold_grads(self, named, named_grads, zero=True):
        """Chain rule from the folded first layers back to the three factors (accumulating, like the library):
        dW1 += M Wf^T + s bf^T, db1 += s, dWf += W1^T M, dbf += W1^T s, with M = dL/d(W1 Wf), s = dL/d(W1 bf + b1)
        (bn_unfold_heads: one launch).  zero: clear M, s afterwards (callers that re-fold before the next backward - the fused
        step - skip it: bn_fold_heads clears them)."""
        if not self.fold_grads:
            return
        named = {k: v.detach() for k, v in named.items()}
        d, _keep = self._fold_desc(named, named_grads)
        L.check(L.lib().bn_unfold_heads(C.byref(d), _stream()), "bn_unfold_heads")
        if zero:
            for m, sv in self.fold_grads.values():
                m.zero_()
                sv.zero_()

    def used_param_names(self):
        names = []
        for l in range(self.layers):
            names += [f"fc_net.{2*l}.weight", f"fc_net.{2*l}.bias"]
        names += ["sigma_from_xyz.0.weight", "sigma_from_xyz.0.bias", "feats_from_xyz.weight", "feats_from_xyz.bias"]
        for name, _, _ in self.heads:
            names += [f"{name}.0.weight", f"{name}.0.bias", f"{name}.2.weight", f"{name}.2.bias"]
        if self.normal_lr:
            names += ["grad_from_xyz.weight", "grad_from_xyz.bias"]
        return names


def make_points(xyz=None, rays=None, z=None, dirs=None, t_embed=None, point_offset=0, total_points=0, z2=None):
    """point_offset / total_points: this call's points inside a larger set that shares one output array and one stash;
    z2 (R, G): the backward over a set of TWO sample blocks of the same rays (bn_points)."""
    pts = L.Points()
    pts.dirs = pts.t_embed = pts.z2 = None
    pts.point_offset, pts.total_points, pts.n_samples2, pts.seg1_points = int(point_offset), int(total_points), 0, 0
    if t_embed is not None:      # per point with xyz, per ray with rays
        rows = xyz.shape[0] if xyz is not None else rays.shape[0]
        assert t_embed.shape[0] == rows and t_embed.is_contiguous() and t_embed.dtype == torch.float32
        pts.t_embed = t_embed.data_ptr()
    if xyz is not None:
        pts.xyz, pts.rays, pts.z = xyz.data_ptr(), None, None
        pts.ray_stride, pts.n_samples, pts.n_points = 0, 0, xyz.shape[0]
        if dirs is not None:
            assert dirs.shape == xyz.shape and dirs.is_contiguous() and dirs.dtype == torch.float32
            pts.dirs = dirs.data_ptr()
    else:
        pts.xyz, pts.rays, pts.z = None, rays.data_ptr(), z.data_ptr()
        pts.ray_stride, pts.n_samples, pts.n_points = rays.shape[1], z.shape[1], z.shape[0] * z.shape[1]
        if z2 is not None:
            assert z2.shape[0] == z.shape[0] and z2.is_contiguous() and z2.dtype == torch.float32
            pts.z2, pts.n_samples2, pts.seg1_points = z2.data_ptr(), z2.shape[1], pts.n_points
            pts.n_points = pts.n_points + z2.shape[0] * z2.shape[1]
    return pts


def pack_field(spec, named_params, packed=None):
    dev = named_params["fc_net.0.weight"].device
    if packed is None:
        packed = torch.empty(spec.packed_bytes, dtype=torch.uint8, device=dev)
    if spec.fold_feats:
        spec.fold(named_params)
    ps = spec.params_struct(named_params)
    L.check(L.lib().bn_pack_field(C.byref(spec.desc), C.byref(ps), _p(packed), _stream()), "bn_pack_field")
    return packed


def field_sigma(spec, named_params, packed, xyz=None, rays=None, z=None, out=None):
    """sigma-only forward, no autograd (pass 1 / sun pass).  out: a caller-owned [n_points] buffer (captured steps)."""
    pts = make_points(xyz, rays, z)
    ref = xyz if xyz is not None else z
    sigma = out if out is not None else torch.empty(pts.n_points, dtype=torch.float32, device=ref.device)
    ps = spec.params_struct(named_params)
    L.check(L.lib().bn_field_sigma(C.byref(spec.desc), C.byref(ps), _p(packed), C.byref(pts), _p(sigma), _stream()),
            "bn_field_sigma")
    return sigma


class FieldFunction(torch.autograd.Function):
    """out[n_points][C] = field(points; params).  Differentiable w.r.t. the parameters and the --beta embedding input
    `t_embed` only (the reference never needs d/d xyz outside the analytic-normal path: z_vals are detached,
    rendering.py:262)."""

    @staticmethod
    def forward(ctx, spec, packed, xyz, rays, z, t_embed, names_grad, *params):
        names, grad_enabled, dirs = names_grad      # grad mode is always off inside Function.forward: passed in
        named = dict(zip(names, params))
        if t_embed is not None:
            t_embed = t_embed.detach().float().contiguous()
        pts = make_points(xyz, rays, z, dirs, t_embed)
        ref = xyz if xyz is not None else z
        out = torch.empty(pts.n_points, spec.out_channels, dtype=torch.float32, device=ref.device)
        ctx.t_grad = bool(grad_enabled and t_embed is not None and ctx.needs_input_grad[5])
        need_grad = grad_enabled and (any(p.requires_grad for p in params) or ctx.t_grad)
        stash = None
        if need_grad or spec.normal_an:
            nbytes = L.lib().bn_field_stash_bytes(C.byref(spec.desc), pts.n_points)
            stash = torch.empty(nbytes, dtype=torch.uint8, device=ref.device)
        ps = spec.params_struct(named)
        L.check(L.lib().bn_field_forward(C.byref(spec.desc), C.byref(ps), _p(packed), C.byref(pts), _p(out), _p(stash),
                                         _stream()), "bn_field_forward")
        if spec.normal_an:
            L.check(L.lib().bn_field_normals(C.byref(spec.desc), C.byref(ps), _p(packed), C.byref(pts), _p(stash), _p(out), None,
                                             1 if need_grad else 0, _stream()), "bn_field_normals")
            if not need_grad:
                stash = None
        ctx.spec, ctx.packed, ctx.names, ctx.stash = spec, packed, names, stash
        ctx.pts_t = (xyz, rays, z, dirs, t_embed)
        ctx.save_for_backward(out, *params)
        return out

    @staticmethod
    def backward(ctx, d_out):
        out, *params = ctx.saved_tensors
        spec, names = ctx.spec, ctx.names
        if ctx.stash is None:
            raise RuntimeError("FieldFunction.backward without a stash (forward ran under no_grad)")
        named = dict(zip(names, params))
        sizes = [p.numel() for p in params]
        offs, tot = [], 0
        for n in sizes:
            offs.append(tot)
            tot += (n + 3) // 4 * 4
        flat = torch.zeros(tot, dtype=torch.float32, device=out.device)
        grads = [flat[o:o + n].view(p.shape) for o, n, p in zip(offs, sizes, params)]
        named_grads = dict(zip(names, grads))
        gs = spec.params_struct(named_grads, grads=True)
        ps = spec.params_struct(named)
        xyz, rays, z, dirs, t_embed = ctx.pts_t
        pts = make_points(xyz, rays, z, dirs, t_embed)
        d_t = None
        if ctx.t_grad:          # per point; the rays form's per-ray gradient is the sum over the ray's samples
            d_t = torch.empty(pts.n_points, spec.t_dim, dtype=torch.float32, device=out.device)
            gs.d_t_embed = d_t.data_ptr()
            if rays is not None:
                d_t = d_t.view(rays.shape[0], -1, spec.t_dim)
        d_out = _f32(d_out)
        L.check(L.lib().bn_field_backward(C.byref(spec.desc), C.byref(ps), _p(ctx.packed), C.byref(pts), _p(out),
                                          _p(d_out), _p(ctx.stash), C.byref(gs), _stream()), "bn_field_backward")
        if spec.fold_feats:
            spec.unfold_grads(named, named_grads)
        ctx.stash = None
        if d_t is not None and d_t.dim() == 3:
            d_t = d_t.sum(1)
        return (None, None, None, None, None, d_t, None) + tuple(g if p.requires_grad else None
                                                                 for g, p in zip(grads, params))


# ----------------------------------------------------------------------------------------- compositing
class CompositeFunction(torch.autograd.Function):
    """(z, out[R,S,C] with sigma in channel 3, noise) -> alphas, transparency, weights, depth, acc[R,C]."""

    @staticmethod
    def forward(ctx, z, out, noise, noise_std):
        R, S = z.shape
        Cc = out.shape[-1] if out.dim() == 3 else 1
        dev = z.device
        alphas = torch.empty(R, S, dtype=torch.float32, device=dev)
        trans = torch.empty_like(alphas)
        weights = torch.empty_like(alphas)
        depth = torch.empty(R, dtype=torch.float32, device=dev)
        sigma_only = out.dim() == 2
        acc = None if sigma_only else torch.empty(R, Cc, dtype=torch.float32, device=dev)
        base = out.data_ptr()
        sig_ptr = C.c_void_p(base if sigma_only else base + 3 * 4)
        L.check(L.lib().bn_composite_forward(_p(z), sig_ptr, 1 if sigma_only else Cc, _p(noise), float(noise_std),
                                             None if sigma_only else _p(out), Cc, 0 if sigma_only else Cc, R, S,
                                             _p(alphas), _p(trans), _p(weights), _p(depth), _p(acc), _stream()),
                "bn_composite_forward")
        ctx.save_for_backward(z, out, noise)
        ctx.noise_std, ctx.sigma_only = float(noise_std), sigma_only
        ctx.mark_non_differentiable(alphas, trans)
        if sigma_only:
            return alphas, trans, weights, depth
        return alphas, trans, weights, depth, acc

    @staticmethod
    def backward(ctx, d_alphas, d_trans, d_weights, d_depth, d_acc=None):
        z, out, noise = ctx.saved_tensors
        R, S = z.shape
        sigma_only = ctx.sigma_only
        Cc = 1 if sigma_only else out.shape[-1]
        d_out = torch.zeros_like(out)
        base = out.data_ptr()
        dbase = d_out.data_ptr()
        sig_ptr = C.c_void_p(base if sigma_only else base + 12)
        dsig_ptr = C.c_void_p(dbase if sigma_only else dbase + 12)
        dw = None if d_weights is None else _f32(d_weights)
        dd = None if d_depth is None else _f32(d_depth)
        da = None if (d_acc is None or sigma_only) else _f32(d_acc)
        L.check(L.lib().bn_composite_backward(_p(z), sig_ptr, 1 if sigma_only else Cc, _p(noise), ctx.noise_std,
                                              None if sigma_only else _p(out), Cc, 0 if sigma_only else Cc, R, S,
                                              _p(dw), _p(dd), _p(da), dsig_ptr, 1 if sigma_only else Cc,
                                              None if sigma_only else _p(d_out), Cc, _stream()),
                "bn_composite_backward")
        return None, d_out, None, None


def composite(z, out, noise=None, noise_std=0.0):
    return CompositeFunction.apply(z.contiguous(), out.contiguous(), noise, noise_std)


def composite_forward_raw(z, out, noise=None, noise_std=0.0, bufs=None):
    """No-autograd compositing of out[R,S,C] (sigma = channel 3): -> alphas, trans, weights, depth, acc.
    `bufs` (optional dict) supplies preallocated outputs so a training loop does not hit the allocator."""
    R, S = z.shape
    Cc = out.shape[-1]
    dev = z.device
    b = bufs if bufs is not None else {}
    mk = lambda k, shape: b.get(k) if k in b else torch.empty(shape, dtype=torch.float32, device=dev)
    alphas, trans, weights = mk("alphas", (R, S)), mk("trans", (R, S)), mk("weights", (R, S))
    depth, acc = mk("depth", (R,)), mk("acc", (R, Cc))
    L.check(L.lib().bn_composite_forward(_p(z), C.c_void_p(out.data_ptr() + 12), Cc, _p(noise), float(noise_std), _p(out), Cc,
                                         Cc, R, S, _p(alphas), _p(trans), _p(weights), _p(depth), _p(acc), _stream()),
            "bn_composite_forward")
    return alphas, trans, weights, depth, acc


def composite_backward_raw(z, out, d_weights, d_depth, d_acc, noise=None, noise_std=0.0, d_out=None):
    """-> d_out[R,S,C].  Channel 3 of d_out receives d sigma; d_acc[:, 3] must be zero (acc[:, 3] is not an output)."""
    R, S = z.shape
    Cc = out.shape[-1]
    if d_out is None:
        d_out = torch.empty_like(out)
    L.check(L.lib().bn_composite_backward(_p(z), C.c_void_p(out.data_ptr() + 12), Cc, _p(noise), float(noise_std), _p(out), Cc,
                                          Cc, R, S, _p(d_weights), _p(d_depth), _p(d_acc),
                                          C.c_void_p(d_out.data_ptr() + 12), Cc, _p(d_out), Cc, _stream()),
            "bn_composite_backward")
    return d_out


def field_forward_raw(spec, named_params, packed, out, stash, xyz=None, rays=None, z=None, point_offset=0, total_points=0):
    """out / stash are the whole SET's when total_points > 0 (this call fills rows [point_offset, point_offset + n_points))."""
    pts = make_points(xyz, rays, z, point_offset=point_offset, total_points=total_points)
    ps = spec.params_struct(named_params)
    L.check(L.lib().bn_field_forward(C.byref(spec.desc), C.byref(ps), _p(packed), C.byref(pts), _p(out), _p(stash), _stream()),
            "bn_field_forward")
    if spec.normal_an:
        L.check(L.lib().bn_field_normals(C.byref(spec.desc), C.byref(ps), _p(packed), C.byref(pts), _p(stash), _p(out), None, 1,
                                         _stream()), "bn_field_normals")
    return out


def field_backward_raw(spec, named_params, named_grads, packed, out, d_out, stash, xyz=None, rays=None, z=None, unfold=True,
                       zero_folded=True, parts=L.BN_BWD_ALL, z2=None):
    """unfold=False leaves the folded first-layer gradients in spec.fold_grads (they keep accumulating): a caller that
    back-propagates several batches before the optimizer step unfolds once, on the last call.  parts: bn_field_backward_parts
    (a caller that overlaps the all-reduce of the trunk's gradient with the rest of the backward).  z2: the points are the two
    sample blocks [z | z2] of the same rays evaluated into one output / stash (field_forward_raw(point_offset=...))."""
    pts = make_points(xyz, rays, z, z2=z2)
    ps, gs = spec.params_struct(named_params), spec.params_struct(named_grads, grads=True)
    L.check(L.lib().bn_field_backward_parts(C.byref(spec.desc), C.byref(ps), _p(packed), C.byref(pts), _p(out), _p(d_out), _p(stash),
                                            C.byref(gs), int(parts), _stream()), "bn_field_backward")
    if spec.fold_feats and unfold:
        spec.unfold_grads(named_params, named_grads, zero=zero_folded)


def field_stash_bytes(spec, n_points):
    return L.lib().bn_field_stash_bytes(C.byref(spec.desc), int(n_points))


def lambert_loss(acc, weights, z, depth, rgbs, rgb_padding, lambda_rgb, valid_depth=None, target_depth=None,
                 target_weight=None, target_std=None, lambda_ds=0.0, usealldepth=False):
    """Shading + SNerfLoss + DepthLoss of a Lambertian step and their gradients in one launch (bn_lambert_loss).
    Returns (loss 0-d, rgb (R,3), d_acc (R,C), d_depth (R), d_weights (R,S))."""
    R, S = weights.shape
    Cc = acc.shape[1]
    dev = acc.device
    ray_loss = torch.empty(R, dtype=torch.float32, device=dev)
    rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
    d_acc = torch.empty(R, Cc, dtype=torch.float32, device=dev)
    d_depth = torch.empty(R, dtype=torch.float32, device=dev)
    d_weights = torch.empty(R, S, dtype=torch.float32, device=dev)
    use = target_depth is not None and lambda_ds > 0
    f = lambda t: _f32(t).contiguous() if (use and t is not None) else None
    # every converted / compacted input stays referenced until the launch has been issued (a temporary freed earlier could
    # be handed to the next conversion by the caching allocator)
    acc, weights, z, depth, rgbs = _f32(acc), _f32(weights), _f32(z), _f32(depth), _f32(rgbs)
    vd, td, tw, ts = f(valid_depth), f(target_depth), f(target_weight), f(target_std)
    L.check(L.lib().bn_lambert_loss(_p(acc), Cc, _p(weights), _p(z), S, _p(depth), _p(rgbs), _p(vd), _p(td), _p(tw), _p(ts),
                                    float(rgb_padding), float(lambda_rgb), float(lambda_ds), int(bool(usealldepth)), R,
                                    _p(ray_loss), _p(rgb), _p(d_acc), _p(d_depth), _p(d_weights), _stream()), "bn_lambert_loss")
    return ray_loss.sum(), rgb, d_acc, d_depth, d_weights


# ----------------------------------------------------------------------------------------- sampling
def stratified_z(near, far, u):
    """near, far: (R,1) (any stride along R), u: (R,S) -> z (R,S)."""
    R, S = u.shape
    near, far, u = _f32(near).reshape(R), _f32(far).reshape(R), _f32(u)
    z = torch.empty(R, S, dtype=torch.float32, device=u.device)
    L.check(L.lib().bn_stratified_z(_p(near), _p(far), 1, _p(u), R, S, _p(z), _stream()), "bn_stratified_z")
    return z


def guided_samples(z, weights, depth, u, near0, far0, d_range, use_target=None, target_depth=None, target_std=None,
                   u_target=None, target_row=None, merge=True):
    """near0 may be a device tensor holding (near0, far0) as two consecutive floats - e.g. rays[0, 6:8] - with far0 = None:
    the kernel then reads the clamp window itself (no device->host read)."""
    R, S = z.shape
    G = u.shape[1]
    dev = z.device
    z2 = torch.empty(R, G, dtype=torch.float32, device=dev)
    z_all = torch.empty(R, S + G, dtype=torch.float32, device=dev) if merge else None
    idx = torch.empty(R, S + G, dtype=torch.int64, device=dev) if merge else None
    if torch.is_tensor(near0):
        assert far0 is None and near0.is_cuda and near0.dtype == torch.float32 and near0.numel() == 2 and near0.is_contiguous()
        L.check(L.lib().bn_guided_samples_nf(_p(z), _p(weights), _p(depth), _p(u), R, S, G, C.c_void_p(near0.data_ptr()),
                                             float(d_range), _p(use_target), _p(target_depth), _p(target_std), _p(u_target),
                                             _p(target_row), _p(z2), _p(z_all), _p(idx), _stream()), "bn_guided_samples_nf")
        return z2, z_all, idx
    L.check(L.lib().bn_guided_samples(_p(z), _p(weights), _p(depth), _p(u), R, S, G, float(near0), float(far0),
                                      float(d_range), _p(use_target), _p(target_depth), _p(target_std), _p(u_target),
                                      _p(target_row), _p(z2), _p(z_all), _p(idx), _stream()), "bn_guided_samples")
    return z2, z_all, idx


# ----------------------------------------------------------------------------------------- launch-lean fused step
def new_step_state(device, seed, lr):
    """Device-resident bn_step_state (include/brdfnerf_hip.h): draw seed / counter, learning rate, Adam step counts, loss ring."""
    st = torch.zeros(L.BN_STATE_BYTES // 8, dtype=torch.int64, device=device)
    st[0] = int(seed) & 0x7FFFFFFFFFFFFFFF
    st.view(torch.float32)[4] = float(lr)
    st.view(torch.float64)[L.BN_STATE_POW_OFF // 8:L.BN_STATE_POW_OFF // 8 + 8] = 1.0          # beta^0
    return st


def set_adam_steps(state, steps, betas=(0.9, 0.999)):
    """Write the per-group optimiser step counts (and the beta powers that go with them) into a step state."""
    steps = list(steps) + [0] * (4 - len(steps))
    state.view(torch.int32)[6:10] = torch.tensor(steps, dtype=torch.int32)
    # the powers of the betas as the kernels receive them (C `float` arguments), as bn_adam_multi's running products hold them
    b1, b2 = (float(torch.tensor(float(b), dtype=torch.float32)) for b in betas)
    pw = [b1 ** s for s in steps] + [b2 ** s for s in steps]
    state.view(torch.float64)[L.BN_STATE_POW_OFF // 8:L.BN_STATE_POW_OFF // 8 + 8] = torch.tensor(pw, dtype=torch.float64)


def state_views(state):
    """(rng_step 0-d int64, lr 0-d float32, adam_step int32[4], loss_ring float32[64]) views of a step state."""
    f, i = state.view(torch.float32), state.view(torch.int32)
    return state[1], f[4], i[6:10], f[L.BN_STATE_LOSS_OFF // 4:L.BN_STATE_LOSS_OFF // 4 + L.BN_STATE_LOSS_SLOTS]


def set_state_noise(state, noise_std):
    """--noise_std of the running step into the device step state (read by the compositing kernels when bn_noise.noise_std < 0)."""
    state.view(torch.float32)[L.BN_STATE_NOISE_OFF // 4].fill_(float(noise_std))


def state_loss_partials(state):
    """The 64 partial sums bn_lambert_tail adds the running step's loss terms to (bn_adam_multi folds them into the ring)."""
    return state.view(torch.float32)[L.BN_STATE_PART_OFF // 4:L.BN_STATE_PART_OFF // 4 + L.BN_STATE_LOSS_SLOTS]


def stratified_z_rng(rays, S, state, z=None, ray_offset=0, near_far=None, stream_id=None):
    """Stratified depths from rays[:, 6], rays[:, 7] - or from near_far [R][2] - with in-kernel uniforms (stream BN_RNG_COARSE of
    `state`, or stream_id)."""
    src, col = (rays, 6) if near_far is None else (near_far, 0)
    R = src.shape[0]
    assert src.is_contiguous() and src.dtype == torch.float32 and src.shape[1] >= col + 2
    if z is None:
        z = torch.empty(R, S, dtype=torch.float32, device=src.device)
    base = src.data_ptr() + 4 * col
    L.check(L.lib().bn_stratified_z_rng(C.c_void_p(base), C.c_void_p(base + 4), src.shape[1], _p(state),
                                        L.BN_RNG_COARSE if stream_id is None else int(stream_id),
                                        int(ray_offset), R, S, _p(z), _stream()), "bn_stratified_z_rng")
    return z


def rng_uniform(state, stream_id, n):
    u = torch.empty(n, dtype=torch.float32, device=state.device)
    L.check(L.lib().bn_rng_uniform(_p(state), int(stream_id), n, _p(u), _stream()), "bn_rng_uniform")
    return u


def rng_normal(state, stream_id, n):
    x = torch.empty(n, dtype=torch.float32, device=state.device)
    L.check(L.lib().bn_rng_normal(_p(state), int(stream_id), n, _p(x), _stream()), "bn_rng_normal")
    return x


def noise_arg(state, noise_std, stream_id, ray_offset=0, from_state=False):
    """bn_noise: --noise_std with in-kernel draws (stream `stream_id` of the step state); None when noise_std == 0.
    from_state: the kernels read the value from the step state (set_state_noise) instead of the launch arguments."""
    if not noise_std:
        return None
    n = L.Noise()
    n.rng, n.noise_std, n.rng_stream, n.ray_offset = state.data_ptr(), -1.0 if from_state else float(noise_std), int(stream_id), int(ray_offset)
    n._keep = state
    return n


def _nz(noise):
    return None if noise is None else C.byref(noise)


def _strided(t):
    """(pointer, element stride) of a 1-d float32 view (e.g. depths[:, 0]); None -> (None, 1)."""
    if t is None:
        return None, 1
    assert t.dtype == torch.float32 and t.dim() == 1 and t.is_cuda
    return C.c_void_p(t.data_ptr()), t.stride(0) if t.shape[0] > 1 else 1


def _rows3(t, R):
    """(R,3) float32 view on the device with unit inner stride (copied when the inner stride is not 1) -> (pointer, row stride);
    None -> (None, 0)."""
    if t is None:
        return None, 0
    assert t.is_cuda and t.dtype == torch.float32 and t.shape == (R, 3)
    if t.stride(1) != 1:
        t = t.contiguous()
    return C.c_void_p(t.data_ptr()), t.stride(0)


def _depth_targets(use, valid_depth, target_depth, target_weight, target_std):
    """The DepthLoss inputs as the kernels take them: (pointer, stride) of each of the four 1-d views in turn, all null with the
    term off."""
    return tuple(a for t in (valid_depth, target_depth, target_weight, target_std) for a in _strided(t if use else None))


def composite_guided(z, out1, G, near_far, d_range, use_target=None, target_depth=None, target_std=None, u=None, u_target=None,
                     state=None, bufs=None, want_pass1=False, ray_offset=0, sigma=None, noise=None):
    """Pass-1 compositing of out1 [R][S][C] (sigma = channel 3; or `sigma` [R][S] from a sigma-only pass 1, out1 = None) +
    depth-guided resampling + merge in one launch.
    Draws: arrays u / u_target [R][G], or the in-kernel streams of `state`.  -> z2 [R][G], z_all [R][S+G], sort_idx [R][S+G]
    (+ pass-1 weights, depth when want_pass1)."""
    R, S = z.shape
    Cc = out1.shape[-1] if sigma is None else 1
    sig_ptr = C.c_void_p(out1.data_ptr() + 12) if sigma is None else _p(sigma)
    dev = z.device
    b = bufs if bufs is not None else {}
    mk = lambda k, shape, dt=torch.float32: b[k] if k in b else torch.empty(shape, dtype=dt, device=dev)
    z2, z_all, idx = mk("z2", (R, G)), mk("z_all", (R, S + G)), mk("idx", (R, S + G), torch.int64)
    w1 = mk("w1", (R, S)) if want_pass1 else None
    d1 = mk("d1", (R,)) if want_pass1 else None
    ut_p, ut_s = _strided(use_target)
    td_p, td_s = _strided(target_depth)
    ts_p, ts_s = _strided(target_std)
    L.check(L.lib().bn_composite_guided(_p(z), sig_ptr, Cc, R, S, G, C.c_void_p(near_far.data_ptr()),
                                        float(d_range), ut_p, ut_s, td_p, td_s, ts_p, ts_s, _p(u), _p(u_target), _p(state),
                                        L.BN_RNG_GUIDED, L.BN_RNG_GUIDED_TARGET, int(ray_offset), _p(z2), _p(z_all), _p(idx), _p(w1), _p(d1),
                                        _nz(noise), _stream()), "bn_composite_guided")
    return (z2, z_all, idx, w1, d1) if want_pass1 else (z2, z_all, idx)


def normal_reg(rays_d, ch_an, ch_lr, lambda_an, lambda_lr, lambda_spv=0.0, spv_ray=None, spv_tot=None):
    """bn_normal_reg: NormalRegLoss (metrics.py:179-216) inside the merged-set compositing; rays_d (R,3) view with unit inner
    stride - and / or NormalLoss 'an_lr' (metrics.py:218-261) between the two normal fields at channels ch_an / ch_lr (lambda_spv
    != 0, with spv_ray [R][2] and spv_tot [4]: see normal_spv_reduce).  None when neither is on."""
    on_an, on_lr = ch_an >= 0 and lambda_an > 0, ch_lr >= 0 and lambda_lr > 0
    on_spv = bool(lambda_spv) and ch_an >= 0 and ch_lr >= 0
    if not (on_an or on_lr or on_spv):
        return None
    nr = L.NormalReg()
    if on_an or on_lr:
        assert rays_d.is_cuda and rays_d.dtype == torch.float32 and rays_d.dim() == 2 and rays_d.stride(1) == 1
        nr.rays_d, nr.rd_stride = rays_d.data_ptr(), rays_d.stride(0)
    nr.ch_an, nr.ch_lr = (ch_an if on_an else -1), (ch_lr if on_lr else -1)
    nr.lambda_an, nr.lambda_lr = float(lambda_an), float(lambda_lr)
    if on_spv:
        nr.lambda_spv, nr.spv_ch_an, nr.spv_ch_lr = float(lambda_spv), int(ch_an), int(ch_lr)
        nr.spv_ray, nr.spv_tot = spv_ray.data_ptr(), spv_tot.data_ptr()
    nr._keep = (rays_d, spv_ray, spv_tot)
    return nr


def normal_spv_reduce(nreg, R, S, ray_loss=None, loss_acc=None):
    """The two batch-wide means of NormalLoss 'an_lr' from the rays' sums (fixed order), the loss term added to the step's loss."""
    _, spv_ray, spv_tot = nreg._keep
    L.check(L.lib().bn_normal_spv_reduce(_p(spv_ray), int(R), int(S), float(nreg.lambda_spv), _p(spv_tot), _p(ray_loss), _p(loss_acc),
                                         _stream()), "bn_normal_spv_reduce")


def merged_composite_forward(z_all, idx, out1, out2, bufs=None, want=("weights", "depth", "acc"), nreg=None, noise=None):
    """Compositing of the depth-sorted union of out1 [R][S1][C] and out2 [R][G][C] read through sort_idx (no cat / gather).
    -> dict with the requested entries of alphas, trans, weights, depth, acc, wsum, var (+ reg: the rays' NormalRegLoss terms,
    with nreg = normal_reg(...))."""
    R, S2 = z_all.shape
    S1, Cc = out1.shape[1], out1.shape[2]
    dev = z_all.device
    b = bufs if bufs is not None else {}
    shapes = dict(alphas=(R, S2), trans=(R, S2), weights=(R, S2), depth=(R,), acc=(R, Cc), wsum=(R,), var=(R,), reg=(R,))
    want = tuple(want) + (("reg",) if (nreg is not None and nreg.rays_d and "reg" not in want) else ())
    o = {k: (b[k] if k in b else torch.empty(shapes[k], dtype=torch.float32, device=dev)) for k in want}
    g = lambda k: _p(o.get(k))
    L.check(L.lib().bn_merged_composite_forward(_p(z_all), _p(idx), _p(out1), _p(out2), S1, S2, Cc, R, g("alphas"), g("trans"),
                                                g("weights"), g("depth"), g("acc"), g("wsum"), g("var"),
                                                None if nreg is None else C.byref(nreg), g("reg") if (nreg is not None and nreg.rays_d) else None,
                                                _nz(noise), _stream()),
            "bn_merged_composite_forward")
    return o


def merged_composite_backward(z_all, idx, out1, out2, d_weights, d_depth, d_acc, d_out1, d_out2, d_wsum=None, nonfinite=None,
                              hs_scale=0.0, depth=None, nreg=None, noise=None):
    """Gradient rows in the SOURCE layouts (d_out1 [R][S1][C], d_out2 [R][G][C]); channel 3 receives d sigma.  hs_scale (with
    the forward's depth): + hs_scale (z - depth)^2 on d loss / d w (HardSurfaceLoss, see ray_shade_loss)."""
    R, S2 = z_all.shape
    S1, Cc = out1.shape[1], out1.shape[2]
    L.check(L.lib().bn_merged_composite_backward(_p(z_all), _p(idx), _p(out1), _p(out2), S1, S2, Cc, R, _p(d_weights), _p(d_depth),
                                                 _p(d_acc), _p(d_wsum), float(hs_scale), _p(depth if hs_scale else None),
                                                 None if nreg is None else C.byref(nreg), _p(d_out1), _p(d_out2), _p(nonfinite),
                                                 _nz(noise), _stream()),
            "bn_merged_composite_backward")


def ray_shade_loss(desc, acc, wsum, depth, var, rays_d, sun_d, rgbs, bufs=None, valid_depth=None, target_depth=None,
                   target_weight=None, target_std=None, ray_loss=None, loss_acc=None, nonfinite=None, extra_loss=None):
    """Ray-level shading + SNerfLoss + DepthLoss + HardSurfaceLoss and their gradients w.r.t. the composited sums in one
    launch (bn_ray_shade_loss).  desc: L.ShadeDesc (rendering.shade_desc).  rays_d / sun_d: (R,3) views with unit inner
    stride (sun_d None: ones).  nonfinite (int64[2]): rays with a non-finite loss term are left out of the step and counted.
    -> dict rgb (R,3), d_acc (R,C), d_wsum (R,), d_depth (R,)."""
    R, Cc = acc.shape
    b = bufs if bufs is not None else {}
    shapes = dict(rgb=(R, 3), d_acc=(R, Cc), d_wsum=(R,), d_depth=(R,))
    o = {k: (b[k] if k in b else torch.empty(sh, dtype=torch.float32, device=acc.device)) for k, sh in shapes.items()}
    dt = _depth_targets(target_depth is not None and desc.lambda_ds > 0, valid_depth, target_depth, target_weight, target_std)
    rdp, rds = _rows3(rays_d, R)
    sdp, sds = _rows3(sun_d, R)
    L.check(L.lib().bn_ray_shade_loss(C.byref(desc), _p(acc), _p(wsum), _p(depth), _p(var), rdp, rds, sdp, sds, _p(rgbs), *dt, R,
                                      _p(o["rgb"]), _p(ray_loss), _p(loss_acc),
                                      0 if loss_acc is None else loss_acc.numel(), _p(o["d_acc"]), _p(o["d_wsum"]), _p(o["d_depth"]),
                                      _p(nonfinite), _p(extra_loss), _stream()), "bn_ray_shade_loss")
    return o


def normal_target_loss(acc, ch, normals, valid_normal, valid_depth, lambda_nr_spv, d_acc, ray_loss=None, loss_acc=None,
                       nonfinite=None, count=None):
    """NormalLoss 'an' / 'lr' (metrics.py:218-261, --nr_spv_type 3 / 2) on the composited normal acc[:, ch:ch+3] against the rays'
    target normals (bn_normal_target_loss): ADDS its gradient into d_acc[:, ch:ch+3] and its per-ray terms into ray_loss /
    loss_acc.  acc, d_acc (R,C) contiguous; normals (R,3) view with unit inner stride; valid_normal, valid_depth (R,) views (any
    stride >= 0).  nonfinite (int64[2]): rays whose term is not finite are left out and counted.  count: int64[1] scratch for the
    number of selected rays (allocated when None).  -> count."""
    R, Cc = acc.shape
    for t in (acc, d_acc):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == (R, Cc)
    np_, ns = _rows3(normals, R)
    vnp, vns = _strided(valid_normal)
    vdp, vds = _strided(valid_depth)
    assert valid_normal.shape[0] == R and valid_depth.shape[0] == R
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=acc.device)
    assert count.is_cuda and count.dtype == torch.int64 and count.numel() >= 1
    L.check(L.lib().bn_normal_target_loss(_p(acc), Cc, int(ch), np_, ns, vnp, vns, vdp, vds, float(lambda_nr_spv), R, _p(d_acc),
                                          _p(ray_loss), _p(loss_acc), 0 if loss_acc is None else loss_acc.numel(), _p(nonfinite),
                                          _p(count), _stream()), "bn_normal_target_loss")
    return count


def ray_shade_dirs(desc, acc, wsum, rays_d, sun, view=None, rgb=None, brdf=None, want_brdf=False):
    """The shading of ray_shade_loss under K directions in one launch (bn_ray_shade_dirs), forward only.  acc (R,C), wsum (R,);
    rays_d (R,3) view with unit inner stride; sun (K,3); view (K,3) or None (-rays_d).  -> rgb (K,R,3) and brdf (K,R,3) or None
    (the value before irradiance and clamp; with `brdf` given or want_brdf)."""
    R, Cc = acc.shape
    K = sun.shape[0]
    for t in (acc, wsum, sun) + (() if view is None else (view,)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert wsum.numel() == R and sun.shape == (K, 3) and (view is None or view.shape == (K, 3)) and desc.C == Cc
    rdp, rds = _rows3(rays_d, R)
    if rgb is None:
        rgb = torch.empty((K, R, 3), dtype=torch.float32, device=acc.device)
    if brdf is None and want_brdf:
        brdf = torch.empty((K, R, 3), dtype=torch.float32, device=acc.device)
    for t in (rgb, brdf):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.shape == (K, R, 3))
    L.check(L.lib().bn_ray_shade_dirs(C.byref(desc), _p(acc), _p(wsum), rdp, rds, _p(sun), _p(view), R, K, _p(rgb), _p(brdf),
                                      _stream()), "bn_ray_shade_dirs")
    return rgb, brdf


# ------------------------------------------------------------------------------ the evaluation entries
def _need(name, t, what, dtype, shape=None, contiguous=True, side=None, cells=None):
    """The one tensor check of the entries that run after training (down to point_normals, and the relighting ones): the C entry
    points see raw pointers, so `t` is a tensor of `dtype` and `shape` or ValueError "<name>: <what> ...", under python -O too.
    shape: a tuple whose int entries must match, ">= n" entries are lower bounds and other strings name free entries; an int: that
    many elements in any shape; None: any.  contiguous: True (required), "copy" / "rows" (a tensor that is not contiguous / whose
    rows do not have unit inner stride is copied, as the wrappers always did) or False (any strides).  side / cells = (lo, hi):
    bounds on every free entry / on their product.  -> t or its copy.  The device is _on_device's, last."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: {what} must be a tensor on the device (there is no host path)")
    if t.dtype != dtype:
        raise ValueError(f"{name}: {what} is {t.dtype}, not {dtype}")
    if isinstance(shape, tuple):
        fits = lambda w, h: h == w if isinstance(w, int) else (not w.startswith(">=") or h >= int(w[2:]))
        ok = t.dim() == len(shape) and all(fits(w, h) for w, h in zip(shape, t.shape))
        form = f"{len(shape)}-D tensor of shape ({', '.join(str(w) for w in shape)})"
    else:
        ok, form = shape is None or t.numel() == shape, "tensor" if shape is None else f"tensor of {shape} elements"
    if not ok or (contiguous is True and not t.is_contiguous()):
        raise ValueError(f"{name}: {what} {tuple(t.shape)} is not a {'contiguous ' if contiguous is True else ''}{form}")
    free = [h for w, h in zip(shape, t.shape) if not isinstance(w, int)] if isinstance(shape, tuple) else []
    for bounds, sizes, unit in ((side, free, "cells a side"), (cells, [math.prod(free)], "cells")):
        if bounds is not None and not all(bounds[0] <= s <= bounds[1] for s in sizes):
            raise ValueError(f"{name}: {what} {tuple(t.shape)} ({bounds[0]} to {bounds[1]} {unit})")
    if contiguous == "copy" or (contiguous == "rows" and t.shape[-1] > 1 and t.stride(-1) != 1):
        return t.contiguous()
    return t


def _maybe(name, t, *spec, **kw):
    """_need for an optional input: None stays None."""
    return None if t is None else _need(name, t, *spec, **kw)


def _out(name, t, what, dtype, shape, device, make=torch.zeros, flat=False):
    """An optional output or accumulator: made (zeroed, unless `make` says otherwise) when None, otherwise checked - by its shape,
    or with `flat` by its number of elements."""
    return make(shape, dtype=dtype, device=device) if t is None else _need(name, t, what, dtype, math.prod(shape) if flat else shape)


def _on_device(name, *tensors):
    """The last of the host-side checks, so that a host tensor is refused by what else is wrong with the call first."""
    if not all(t.is_cuda for t in tensors if t is not None):
        raise ValueError(f"{name}: every tensor must be on the device (there is no host path)")


def _rows(name, H, rows):
    """rows = (row0, row1), or None for all H rows, of a grid entry -> (row0, row1), or ValueError by name outside [0, H]."""
    row0, row1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= row0 <= row1 <= H:
        raise ValueError(f"{name}: rows ({row0}, {row1}) outside [0, {H}]")
    return row0, row1


F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
FILL_GRID = dict(shape=("H", "W"), side=(1, L.BN_FILL_MAX_SIDE))                          # a grid of the hole filling
VIS_DSM = dict(what="dsm", dtype=F32, shape=("H", "W"), cells=(1, 1 << 30))               # the height grid of the visibility entries
VIS_POINTS = dict(what="points", dtype=F64, shape=("R", 3), contiguous="copy", cells=(0, 1 << 30))      # point_cloud's output


def fixed_mean(total, count, fix):
    """The mean that an integer (sum of llrint(v fix), count) pair stands for; Python integers in, NaN for a zero count."""
    return total / (count * fix) if count else float("nan")


def _ray_rows(name, rays, depth):
    """rays (R, >= 6) float32 rows with unit inner stride and depth (R,) float32, copied where they are not -> rays, depth, R and
    the row stride."""
    rays = _need(name, rays, "rays", F32, ("R", ">=6"), "rows")
    R = rays.shape[0]
    depth = _need(name, depth, "depth", F32, (R,), "copy")
    return rays, depth, R, (rays.stride(0) if R > 1 else rays.shape[1])       # (one row: its stride is not read)


def _dsm_acc(name, acc, skipped, *others):
    """The (H, W, 2) int64 accumulator and the (1,) int64 counter of the DSM splats, then the device of all -> H, W."""
    _need(name, acc, "acc", I64, ("H", "W", 2))
    _need(name, skipped, "skipped", I64, 1)
    _on_device(name, acc, skipped, *others)
    return acc.shape[0], acc.shape[1]


def dsm_splat(rays, depth, center, rng, xoff, yoff, resolution, radius, footprint, acc, skipped):
    """The depths of R rays splatted into a DSM accumulator (bn_dsm_splat).  rays (R, >= 6) float32 rows with unit inner stride
    (origin, direction), depth (R,) float32; center (3 floats) and rng the scene normalisation, (xoff, yoff) the grid's north-west
    corner; acc (H, W, 2) int64 = (sum, count) and skipped (1,) int64 on the device, accumulated into."""
    rays, depth, R, stride = _ray_rows("dsm_splat", rays, depth)
    H, W = _dsm_acc("dsm_splat", acc, skipped, rays, depth)
    if R == 0:
        return acc
    with torch.cuda.device(rays.device):
        L.check(L.lib().bn_dsm_splat(C.c_void_p(rays.data_ptr()), stride, _p(depth), R,
                                     *_abi_args((center, rng), (xoff, yoff, resolution, W, H, radius, footprint)), _p(acc), _p(skipped),
                                     _stream()), "bn_dsm_splat")
    return acc


def _abi_args(frame=(), grid=(), world=()):
    """The arguments the surface-model entries share, in ABI order: frame (center, rng) -> center[3], range; grid (xoff, yoff,
    resolution, W, H, radius, footprint); world (cs, zone, south).  An entry passes the parts it takes."""
    frame = ((C.c_double * 3)(*[float(v) for v in frame[0]]), float(frame[1])) if frame else ()
    return frame + tuple(float(v) for v in grid[:3]) + tuple(int(v) for v in grid[3:]) + tuple(int(v) for v in world)


def ecef_geodetic(xyz, skipped):
    """Geodetic points of ECEF points (bn_ecef_geodetic): xyz (n, 3) float64 -> lonlat (n, 2) in degrees, alt (n,) float64, NaN
    where a point is refused (on the axis or not finite); skipped (1,) int64 on the device, accumulated into."""
    xyz = _need("ecef_geodetic", xyz, "xyz", F64, ("n", 3), "copy")
    _need("ecef_geodetic", skipped, "skipped", I64, 1)
    _on_device("ecef_geodetic", xyz, skipped)
    n = xyz.shape[0]
    lonlat = torch.empty((n, 2), dtype=torch.float64, device=xyz.device)
    alt = torch.empty((n,), dtype=torch.float64, device=xyz.device)
    if n == 0:
        return lonlat, alt
    with torch.cuda.device(xyz.device):
        L.check(L.lib().bn_ecef_geodetic(_p(xyz), n, _p(lonlat), _p(alt), _p(skipped), _stream()), "bn_ecef_geodetic")
    return lonlat, alt


def surface_points(rays, depth, center, rng, cs, zone, south, skipped):
    """(east, north, altitude) of R rays' surface points (bn_surface_points): rays (R, >= 6) float32 rows with unit inner stride,
    depth (R,) float32; cs BN_CS_ECEF or BN_CS_UTM, the scene's zone -> float64 (R, 3), NaN where a row is refused; skipped (1,)
    int64 on the device, accumulated into."""
    rays, depth, R, stride = _ray_rows("surface_points", rays, depth)
    _need("surface_points", skipped, "skipped", I64, 1)
    _on_device("surface_points", rays, depth, skipped)
    enz = torch.empty((R, 3), dtype=torch.float64, device=rays.device)
    if R == 0:
        return enz
    with torch.cuda.device(rays.device):
        L.check(L.lib().bn_surface_points(C.c_void_p(rays.data_ptr()), stride, _p(depth), R,
                                          *_abi_args((center, rng), world=(cs, zone, south)), _p(enz), _p(skipped), _stream()),
                "bn_surface_points")
    return enz


def dsm_splat_points(enz, xoff, yoff, resolution, radius, footprint, acc, skipped):
    """World points that already are (east, north, altitude) splatted into a DSM accumulator (bn_dsm_splat_points): enz (n, >= 3)
    float64 rows with unit inner stride; acc and skipped as dsm_splat."""
    enz = _need("dsm_splat_points", enz, "enz", F64, ("n", ">=3"), "rows")
    H, W = _dsm_acc("dsm_splat_points", acc, skipped, enz)
    if enz.shape[0] == 0:
        return acc
    with torch.cuda.device(enz.device):
        L.check(L.lib().bn_dsm_splat_points(C.c_void_p(enz.data_ptr()), enz.stride(0) if enz.shape[0] > 1 else enz.shape[1], enz.shape[0],
                                            *_abi_args(grid=(xoff, yoff, resolution, W, H, radius, footprint)), _p(acc), _p(skipped),
                                            _stream()), "bn_dsm_splat_points")
    return acc


def dsm_splat_world(rays, depth, center, rng, xoff, yoff, resolution, radius, footprint, cs, zone, south, acc, skipped):
    """dsm_splat for a scene whose world points are `cs` (bn_dsm_splat_world): ray -> world point -> (east, north, altitude) ->
    deposit in one launch."""
    rays, depth, R, stride = _ray_rows("dsm_splat_world", rays, depth)
    H, W = _dsm_acc("dsm_splat_world", acc, skipped, rays, depth)
    if R == 0:
        return acc
    with torch.cuda.device(rays.device):
        L.check(L.lib().bn_dsm_splat_world(C.c_void_p(rays.data_ptr()), stride, _p(depth), R,
                                           *_abi_args((center, rng), (xoff, yoff, resolution, W, H, radius, footprint), (cs, zone, south)),
                                           _p(acc), _p(skipped), _stream()), "bn_dsm_splat_world")
    return acc


def ortho_top(rays, depth, center, rng, xoff, yoff, resolution, radius, footprint, cs, zone, south, top, skipped):
    """Pass 1 of the orthorectified maps (bn_ortho_top): top (H, W) int64, filled with BN_ORTHO_EMPTY by the caller, takes the
    maximum of the quantised altitudes over every ray's footprint; rays, depth, the frame and the grid as dsm_splat_world; skipped
    (1,) int64 on the device, accumulated into."""
    rays, depth, R, stride = _ray_rows("ortho_top", rays, depth)
    _need("ortho_top", top, "top", I64, ("H", "W"))
    _need("ortho_top", skipped, "skipped", I64, 1)
    _on_device("ortho_top", rays, depth, top, skipped)
    if R == 0:
        return top
    H, W = top.shape
    with torch.cuda.device(rays.device):
        L.check(L.lib().bn_ortho_top(C.c_void_p(rays.data_ptr()), stride, _p(depth), R,
                                     *_abi_args((center, rng), (xoff, yoff, resolution, W, H, radius, footprint), (cs, zone, south)),
                                     _p(top), _p(skipped), _stream()), "bn_ortho_top")
    return top


def ortho_splat(rays, depth, center, rng, xoff, yoff, resolution, radius, footprint, cs, zone, south, features, top, band_q, acc,
                counters):
    """Pass 2 of the orthorectified maps (bn_ortho_splat): features (R, E) float32 rows with unit channel stride (a column slice of
    a wider tensor is read in place; None with E == 0) deposited with the altitude into acc (H, W, 2 + E) int64 = (sum_z, count,
    sum_0 ...), accumulated into; top (H, W) int64 of ortho_top or None (mean mode), band_q in units of 2^-20 m; counters (3,)
    int64 on the device = (bad points, bad features, culled deposits), accumulated into."""
    name = "ortho_splat"
    rays, depth, R, stride = _ray_rows(name, rays, depth)
    _need(name, acc, "acc", I64, ("H", "W", ">=2"))
    H, W, E = acc.shape[0], acc.shape[1], acc.shape[2] - 2
    _need(name, counters, "counters", I64, 3)
    _maybe(name, top, "top", I64, (H, W))
    if E == 0:
        if features is not None and tuple(features.shape) != (R, 0):
            raise ValueError(f"{name}: features {tuple(features.shape)} for an accumulator without channels")
        features = None
    else:
        features = _need(name, features, "features", F32, (R, E), "rows")
    _on_device(name, rays, depth, acc, counters, top, features)
    fp = None if E == 0 else C.c_void_p(features.data_ptr())
    fs = 0 if E == 0 else (features.stride(0) if R > 1 else E)       # (one row: its stride is not read)
    if R == 0:
        return acc
    with torch.cuda.device(rays.device):
        L.check(L.lib().bn_ortho_splat(C.c_void_p(rays.data_ptr()), stride, _p(depth), R,
                                       *_abi_args((center, rng), (xoff, yoff, resolution, W, H, radius, footprint), (cs, zone, south)),
                                       fp, fs, E, _p(top), int(band_q), _p(acc), _p(counters), _stream()), "bn_ortho_splat")
    return acc


def ortho_resolve(acc, want_count=True):
    """The means of an accumulator of orthorectified maps (bn_ortho_resolve): acc (H, W, 2 + E) int64 -> maps (E, H, W) float32,
    dsm (H, W) float32, both NaN where no point fell, and count (H, W) int32 (or None)."""
    _need("ortho_resolve", acc, "acc", I64, ("H", "W", ">=2"))
    _on_device("ortho_resolve", acc)
    H, W, E = acc.shape[0], acc.shape[1], acc.shape[2] - 2
    maps = torch.empty((E, H, W), dtype=torch.float32, device=acc.device)
    dsm = torch.empty((H, W), dtype=torch.float32, device=acc.device)
    count = torch.empty((H, W), dtype=torch.int32, device=acc.device) if want_count else None
    with torch.cuda.device(acc.device):
        L.check(L.lib().bn_ortho_resolve(_p(acc), W, H, E, _p(maps) if E else None, _p(dsm), _p(count), _stream()), "bn_ortho_resolve")
    return maps, dsm, count


def dsm_resolve(acc, want_count=True):
    """Mean altitude per cell of a DSM accumulator (bn_dsm_resolve): acc (H, W, 2) int64 -> dsm (H, W) float32, NaN where no
    point fell, and count (H, W) int32 (or None)."""
    _need("dsm_resolve", acc, "acc", I64, ("H", "W", 2))
    _on_device("dsm_resolve", acc)
    H, W = acc.shape[0], acc.shape[1]
    dsm = torch.empty((H, W), dtype=torch.float32, device=acc.device)
    count = torch.empty((H, W), dtype=torch.int32, device=acc.device) if want_count else None
    with torch.cuda.device(acc.device):
        L.check(L.lib().bn_dsm_resolve(_p(acc), W, H, _p(dsm), _p(count), _stream()), "bn_dsm_resolve")
    return dsm, count


def ssim_map(pred, gt, C_, H, W, strides, mask, div, max_val, window, g, sums, rows=None, out=None):
    """The SSIM index map of two images and its integer sum (bn_ssim_map).  pred, gt: contiguous float32 device buffers read
    through the element strides (plane, row, col) - no copy; mask (H, W) uint8 or None; g the `window` float64 Gaussian weights;
    sums (3,) int64 = (sum of llrint(v 2^30), cells summed, cells skipped), accumulated into; rows = (row0, row1) output rows
    (default all); out (C, H, W) float32 map or None."""
    sp, sr, sc = (int(s) for s in strides)
    last = (C_ - 1) * sp + (H - 1) * sr + (W - 1) * sc
    for t, what in ((pred, "pred"), (gt, "gt")):
        _need("ssim_map", t, what, F32)
        if min(sp, sr, sc) < 0 or last >= t.numel():
            raise ValueError(f"ssim_map: {what} of {t.numel()} elements is read through the strides {(sp, sr, sc)} up to element {last}")
    _maybe("ssim_map", mask, "mask", U8, (H, W))
    _need("ssim_map", sums, "sums", I64, 3)
    _maybe("ssim_map", out, "out", F32, (C_, H, W))
    if len(g) != window:
        raise ValueError(f"ssim_map: {len(g)} weights for a window of {window}")
    _on_device("ssim_map", pred, gt, mask, sums, out)
    row0, row1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
    gw = (C.c_double * window)(*[float(v) for v in g])
    L.check(L.lib().bn_ssim_map(_p(pred), _p(gt), C_, H, W, sp, sr, sc, _p(mask), float(div), float(max_val), int(window), gw, row0, row1,
                                _p(out), _p(sums), _stream()), "bn_ssim_map")
    return sums


def grid_normals(z, resolution):
    """The reference's four-cross-product normals of an altitude grid (bn_grid_normals): z (H, W) float32 -> (H, W, 3) float32,
    zero on the border.  y grows with the row, as upstream: flat ground gives (0, 0, -1)."""
    z = _need("grid_normals", z, "z", F32, ("H", "W"), "copy")
    _on_device("grid_normals", z)
    H, W = z.shape
    out = torch.empty((H, W, 3), dtype=torch.float32, device=z.device)
    L.check(L.lib().bn_grid_normals(_p(z), H, W, float(resolution), _p(out), _stream()), "bn_grid_normals")
    return out


def normal_angle(n1, n2, mask=None, border=0, sums=None, want_map=True):
    """The angle in degrees between two normal grids (bn_normal_angle): n1, n2 (H, W, 3) float32, mask (H, W) uint8 (nonzero:
    inside) or None -> angle (H, W) float32 (or None), sums (6,) int64 = (sum of llrint(a 2^20), count) over all, inside and
    outside cells, NaN cells left out.  border 0: the reference's (zero border normals: 90 degrees); 1: the border is NaN."""
    name = "normal_angle"
    H, W = _need(name, n1, "n1", F32, ("H", "W", 3)).shape[:2]
    _need(name, n2, "n2", F32, (H, W, 3))
    _maybe(name, mask, "mask", U8, (H, W))
    sums = _out(name, sums, "sums", I64, (6,), n1.device, flat=True)
    _on_device(name, n1, n2, mask, sums)
    angle = torch.empty((H, W), dtype=torch.float32, device=n1.device) if want_map else None
    L.check(L.lib().bn_normal_angle(_p(n1), _p(n2), H, W, _p(mask), int(border), _p(angle), _p(sums), _stream()), "bn_normal_angle")
    return angle, sums


def grid_halve(src):
    """One level of the registration pyramid (bn_grid_halve): src (H, W) float64 -> (ceil(H / 2), ceil(W / 2)) float64, the mean of
    the finite cells of upstream's 2 x 2 box, NaN where there is none."""
    src = _need("grid_halve", src, "src", F64, ("H", "W"), "copy")
    _on_device("grid_halve", src)
    H, W = src.shape
    out = torch.empty(((H + 1) // 2, (W + 1) // 2), dtype=torch.float64, device=src.device)
    L.check(L.lib().bn_grid_halve(_p(src), H, W, _p(out), _stream()), "bn_grid_halve")
    return out


def ncc_moments(u, v, pivot, k, dx0, dy0, r, sums=None, skipped=None, rows=None):
    """The integer moments of every shift of a (2r + 1)^2 window around (dx0, dy0) (bn_ncc_moments): u, v (H, W) float64 on the
    device -> sums ((2r + 1)^2, 6) int64 = (N, Su, Sv, Suu, Svv, Suv) in scan order (dy outer, dx inner) and skipped (1,) int64,
    both accumulated into when given; rows = (row0, row1) rows of u (default all)."""
    name = "ncc_moments"
    H, W = _need(name, u, "u", F64, ("H", "W")).shape
    _need(name, v, "v", F64, (H, W))
    n = (2 * int(r) + 1) ** 2 if 0 <= int(r) <= L.BN_NCC_MAX_RANGE else 1          # a refused r never reaches the kernel
    sums = _out(name, sums, "sums", I64, (n, 6), u.device, flat=True)
    skipped = _out(name, skipped, "skipped", I64, (1,), u.device, flat=True)
    _on_device(name, u, v, sums, skipped)
    row0, row1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
    L.check(L.lib().bn_ncc_moments(_p(u), _p(v), H, W, float(pivot), int(k), int(dx0), int(dy0), int(r), row0, row1, _p(sums),
                                   _p(skipped), _stream()), "bn_ncc_moments")
    return sums, skipped


def dsm_shift_diff(pred, gt, dx, dy, b, mask=None, sums=None, want_maps=True):
    """A DSM shifted by (dx, dy) cells and b metres and its difference to the ground truth (bn_dsm_shift_diff): pred, gt (H, W)
    float32, mask (H, W) uint8 (nonzero: inside) or None -> rdsm, diff (H, W) float32 (or None, None), sums (6,) int64 = (sum of
    llrint(|diff| 2^20), count) over all, inside and outside cells, NaN cells left out."""
    name = "dsm_shift_diff"
    H, W = _need(name, pred, "pred", F32, ("H", "W")).shape
    _need(name, gt, "gt", F32, (H, W))
    _maybe(name, mask, "mask", U8, (H, W))
    sums = _out(name, sums, "sums", I64, (6,), pred.device, flat=True)
    _on_device(name, pred, gt, mask, sums)
    rdsm = torch.empty((H, W), dtype=torch.float32, device=pred.device) if want_maps else None
    diff = torch.empty((H, W), dtype=torch.float32, device=pred.device) if want_maps else None
    L.check(L.lib().bn_dsm_shift_diff(_p(pred), _p(gt), H, W, int(dx), int(dy), float(b), _p(mask), _p(rdsm), _p(diff), _p(sums),
                                      _stream()), "bn_dsm_shift_diff")
    return rdsm, diff, sums


def grid_nearest_col(src):
    """The column pass of the hole filling (bn_grid_nearest_col): src (H, W) float32 -> near_row (H, W) int32, per cell the row of
    the nearest known (not NaN) cell of its column, ties to the smaller row, -1 in a column without one."""
    _need("grid_nearest_col", src, "src", F32, **FILL_GRID)
    _on_device("grid_nearest_col", src)
    H, W = src.shape
    near_row = torch.empty((H, W), dtype=torch.int32, device=src.device)
    L.check(L.lib().bn_grid_nearest_col(_p(src), H, W, _p(near_row), _stream()), "bn_grid_nearest_col")
    return near_row


def grid_fill(src, near_row, rows=None, want_source=False, want_dist2=False):
    """The row pass of the hole filling (bn_grid_fill): src (H, W) float32 and its grid_nearest_col -> dst (H, W) float32 (every cell
    the bits of its nearest known cell), source (H, W) int32 flat index of that cell and dist2 (H, W) int32 (or None), counts (2,)
    int64 = (holes, largest d2).  rows = (row0, row1): only those rows are written (the others are uninitialised) and counted."""
    _need("grid_fill", src, "src", F32, **FILL_GRID)
    _need("grid_fill", near_row, "near_row", I32, **FILL_GRID)
    if near_row.shape != src.shape:
        raise ValueError(f"grid_fill: near_row {tuple(near_row.shape)} is not on the grid {tuple(src.shape)}")
    H, W = src.shape
    row0, row1 = _rows("grid_fill", H, rows)
    _on_device("grid_fill", src, near_row)
    dst = torch.empty((H, W), dtype=torch.float32, device=src.device)
    source = torch.empty((H, W), dtype=torch.int32, device=src.device) if want_source else None
    dist2 = torch.empty((H, W), dtype=torch.int32, device=src.device) if want_dist2 else None
    counts = torch.zeros((2,), dtype=torch.int64, device=src.device)
    L.check(L.lib().bn_grid_fill(_p(src), _p(near_row), H, W, row0, row1, _p(dst), _p(source), _p(dist2), _p(counts), _stream()),
            "bn_grid_fill")
    return dst, source, dist2, counts


def _vis_dirs(name, dirs):
    """(K, 3) or (3,) directions in any float dtype -> (K, 3) float64 on the HOST (the entries check them there), K in
    [1, BN_VIS_MAX_DIRS], every component finite and dz > 0, or ValueError by name."""
    dirs = torch.as_tensor(dirs)
    if not dirs.is_floating_point():
        raise ValueError(f"{name}: dirs are {dirs.dtype}, not a float dtype")
    dirs = dirs.detach().to(device="cpu", dtype=torch.float64)
    if dirs.dim() == 1 and dirs.numel() == 3:
        dirs = dirs.reshape(1, 3)
    if dirs.dim() != 2 or dirs.shape[1] != 3 or not 1 <= dirs.shape[0] <= L.BN_VIS_MAX_DIRS:
        raise ValueError(f"{name}: dirs {tuple(dirs.shape)} are not (K, 3) or (3,) with K from 1 to {L.BN_VIS_MAX_DIRS}")
    if not bool(torch.isfinite(dirs).all()) or not bool((dirs[:, 2] > 0).all()):
        raise ValueError(f"{name}: every direction must be finite and point above the horizon (dz > 0)")
    return dirs.contiguous()


def _vis_scalars(name, res, eps, zmax):
    res, eps, zmax = float(res), float(eps), float(zmax)
    if not (res > 0 and math.isfinite(res)):
        raise ValueError(f"{name}: resolution {res} must be positive and finite")
    if not (eps >= 0 and math.isfinite(eps)):
        raise ValueError(f"{name}: eps {eps} must be finite and not negative")
    if math.isnan(zmax):
        raise ValueError(f"{name}: zmax is NaN")
    return res, eps, zmax


def grid_visibility(dsm, res, dirs, eps=0.0, zmax=float("inf"), rows=None, vis=None, hit=None, counts=None, want_hit=False):
    """The visibility of the cells of a height grid (bn_grid_visibility): dsm (H, W) float32 on the device, dirs (K, 3) (east,
    north, up) towards the sun or the sensor, taken to float64 on the host.  rows = (row0, row1): only those rows are written (the
    others are uninitialised unless `vis` / `hit` come in) and counted.  vis (K, H, W) uint8, hit (K, H, W) int32 and counts (K, 3)
    int64 may be given - counts are accumulated into.  -> vis, hit or None (want_hit, or `hit` given), counts."""
    name = "grid_visibility"
    _need(name, dsm, **VIS_DSM)
    dirs = _vis_dirs(name, dirs)
    res, eps, zmax = _vis_scalars(name, res, eps, zmax)
    H, W = dsm.shape
    K = dirs.shape[0]
    row0, row1 = _rows(name, H, rows)
    vis = _out(name, vis, "vis", U8, (K, H, W), dsm.device, torch.empty)
    if hit is not None or want_hit:
        hit = _out(name, hit, "hit", I32, (K, H, W), dsm.device, torch.empty)
    counts = _out(name, counts, "counts", I64, (K, 3), dsm.device)
    _on_device(name, dsm, vis, hit, counts)
    L.check(L.lib().bn_grid_visibility(_p(dsm), H, W, res, row0, row1, dirs.numpy().ctypes.data_as(C.POINTER(C.c_double)), K, eps, zmax,
                                       _p(vis), _p(hit), _p(counts), _stream()), "bn_grid_visibility")
    return vis, hit, counts


def points_visibility(points, dsm, xoff, yoff, res, dirs, eps=0.0, zmax=float("inf"), want_hit=False):
    """The visibility of world points over a height grid (bn_points_visibility): points (R, 3) float64 (east, north, altitude) on
    the device (point_cloud's output), dsm (H, W) float32 with its Grid's origin and resolution, dirs (K, 3).
    -> vis (K, R) uint8, hit (K, R) int32 or None, counts (K, 3) int64."""
    name = "points_visibility"
    points = _need(name, points, **VIS_POINTS)
    _need(name, dsm, **VIS_DSM)
    dirs = _vis_dirs(name, dirs)
    res, eps, zmax = _vis_scalars(name, res, eps, zmax)
    xoff, yoff = float(xoff), float(yoff)
    if not (math.isfinite(xoff) and math.isfinite(yoff)):
        raise ValueError(f"{name}: grid origin ({xoff}, {yoff}) is not finite")
    _on_device(name, points, dsm)
    H, W = dsm.shape
    R, K = points.shape[0], dirs.shape[0]
    vis = torch.empty((K, R), dtype=torch.uint8, device=dsm.device)
    hit = torch.empty((K, R), dtype=torch.int32, device=dsm.device) if want_hit else None
    counts = torch.zeros((K, 3), dtype=torch.int64, device=dsm.device)
    if R:
        L.check(L.lib().bn_points_visibility(_p(points), R, _p(dsm), H, W, xoff, yoff, res, dirs.numpy().ctypes.data_as(C.POINTER(C.c_double)),
                                             K, eps, zmax, _p(vis), _p(hit), _p(counts), _stream()), "bn_points_visibility")
    return vis, hit, counts


RAY_MAP_COUNTERS = ("std_sum", "std_count", "std_skipped", "bad_nr", "nr0", "nr_total")


def ray_maps(z_vals, weights, depth, X=None, accumulate=False, normal_col=None, view=None, counters=None, want_surf=True):
    """The per-ray reductions over the depth-sorted samples (bn_ray_maps).  z_vals, weights (R, S) and depth (R,) float32,
    contiguous; X (R, S, E) float32 with any non-negative strides (a column slice of the field rows is read in place) or None;
    normal_col: the first of three channels of X holding a normal, with view (R, 3) float32 = -rays_d (unit inner stride).
    counters (6,) int64 is accumulated into when given (RAY_MAP_COUNTERS names its entries).
    -> surf_idx (R,) int32, surf (R, E) or None, var (R,), std (R,), accum (R, E) or None, counters."""
    name = "ray_maps"
    R, S = _need(name, z_vals, "z_vals", F32, ("R", "S")).shape
    _need(name, weights, "weights", F32, (R, S))
    _need(name, depth, "depth", F32, (R,))
    if not 1 <= S <= L.BN_MAPS_MAX_SAMPLES:
        raise ValueError(f"{name}: S = {S} samples (1 to {L.BN_MAPS_MAX_SAMPLES})")
    E = 0
    if X is not None:
        E = _need(name, X, "X", F32, (R, S, "E"), False).shape[2]
        if not 0 <= E <= L.BN_MAPS_MAX_CHANNELS:
            raise ValueError(f"{name}: X has E = {E} channels (0 to {L.BN_MAPS_MAX_CHANNELS})")
        if any(st < 0 for st in X.stride()):
            raise ValueError(f"{name}: X has a negative stride {tuple(X.stride())}")
    if accumulate and E == 0:
        raise ValueError(f"{name}: accumulate=True needs a per-sample tensor X with at least one channel")
    nc = -1
    if normal_col is not None:
        nc = int(normal_col)
        if not 0 <= nc <= E - 3:
            raise ValueError(f"{name}: normal column {nc} outside [0, E - 3] with E = {E}")
        if view is None:
            raise ValueError(f"{name}: a normal column needs the view vectors (view = -rays_d)")
        view = _need(name, view, "view", F32, (R, 3), "rows")
    dev = z_vals.device
    counters = _out(name, counters, "counters", I64, (len(RAY_MAP_COUNTERS),), dev, flat=True)
    _on_device(name, z_vals, weights, depth, counters, X, view if nc >= 0 else None)
    surf_idx = torch.empty((R,), dtype=torch.int32, device=dev)
    var, std = torch.empty((R,), dtype=torch.float32, device=dev), torch.empty((R,), dtype=torch.float32, device=dev)
    surf = torch.empty((R, E), dtype=torch.float32, device=dev) if (E and want_surf) else None
    accum = torch.empty((R, E), dtype=torch.float32, device=dev) if accumulate else None
    raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    xr, xs, xc = (0, 0, 0) if (X is None or E == 0) else X.stride()
    L.check(L.lib().bn_ray_maps(_p(z_vals), _p(weights), _p(depth), raw(X) if E else None, xr, xs, xc, nc, raw(view) if nc >= 0 else None,
                                view.stride(0) if nc >= 0 else 0, R, S, E, _p(surf_idx), _p(surf), _p(var), _p(std), _p(accum),
                                _p(counters), _stream()), "bn_ray_maps")
    return surf_idx, surf, var, std, accum, counters


def point_normals(points, valid=None, round_f32=True):
    """The normals of an (H, W, 3) float64 image of points (bn_point_normals): -> normals (H, W, 3) float32, zero on the border, and
    valid_out (H, W) float32 or None (with valid (H, W) float32).  round_f32: the reference's float32 points."""
    name = "point_normals"
    points = _need(name, points, "the image of points", F64, ("H", "W", 3), "copy", cells=(1, 1 << 30))
    H, W = points.shape[:2]
    valid = _maybe(name, valid, "valid", F32, (H, W), "copy")
    _on_device(name, points, valid)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=points.device)
    valid_out = None if valid is None else torch.empty((H, W), dtype=torch.float32, device=points.device)
    L.check(L.lib().bn_point_normals(_p(points), H, W, int(bool(round_f32)), _p(valid), _p(out), _p(valid_out), _stream()),
            "bn_point_normals")
    return out, valid_out


def sample_shade_dirs(desc, X, w, rays_d, sun, view=None, rgb=None, brdf=None, want_brdf=False):
    """ray_shade_dirs for one BRDF per sample (bn_sample_shade_dirs), forward only.  X (R,S,C) depth-sorted field-output rows,
    w (R,S) their weights; rays_d (R,3) view with unit inner stride; sun (K,3); view (K,3) or None (-rays_d).  rgb / brdf: (K,R,3)
    float32 on the device, rows contiguous - the planes may be further apart (a (K, i:j, 3) slice of a whole view).
    -> rgb (K,R,3) and brdf (K,R,3) = sum_s w brdf_s or None (with `brdf` given or want_brdf)."""
    name = "sample_shade_dirs"
    R, S = _need(name, X, "X", F32, ("R", "S", int(desc.C))).shape[:2]
    _need(name, w, "w", F32, (R, S))
    K = _need(name, sun, "sun", F32, ("K", 3)).shape[0]
    _maybe(name, view, "view", F32, (K, 3))
    rays_d = _need(name, rays_d, "rays_d", F32, (R, 3), "rows")
    if rgb is None:
        rgb = torch.empty((K, R, 3), dtype=torch.float32, device=X.device)
    if brdf is None and want_brdf:
        brdf = torch.empty((K, R, 3), dtype=torch.float32, device=X.device)
    planes = []
    for t, what in ((rgb, "rgb"), (brdf, "brdf")):
        if t is not None and not plane_rows(_need(name, t, what, F32, (K, R, 3), False)):
            raise ValueError(f"{name}: {what} with strides {t.stride()}: its (R, 3) planes must be contiguous rows that do not overlap")
        planes.append(3 * R if (t is None or K == 1) else t.stride(0))
    _on_device(name, X, w, sun, view, rays_d, rgb, brdf)
    rdp, rds = _rows3(rays_d, R)
    raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L.check(L.lib().bn_sample_shade_dirs(C.byref(desc), _p(X), _p(w), rdp, rds, _p(sun), _p(view), R, S, K, raw(rgb), planes[0],
                                         raw(brdf), planes[1], _stream()), "bn_sample_shade_dirs")
    return rgb, brdf


def plane_rows(t):
    """(K,R,3) whose (R,3) planes are contiguous rows and do not overlap: what bn_sample_shade_dirs writes through a plane stride."""
    K, R, _ = t.shape
    return R == 0 or ((t.stride(2) == 1 and (R == 1 or t.stride(1) == 3)) and (K == 1 or t.stride(0) >= 3 * R))


def sun_ray_table(rays, d1, sun, u, table=None, z_sun=None):
    """Rays and depths of the sun-visibility pass for K directions in one launch (bn_sun_ray_table).  rays (R, >= 6) float32
    contiguous, d1 (R,) the pass-1 depth, sun (K, 3), u (R, G) the pass's uniforms, shared by all K.  -> table (K R, 8) rows
    (surface point, sun_k, 0.01 far, far) and z_sun (K R, G): what field_sigma(rays=table, z=z_sun) takes; per direction bitwise
    rendering.sun_far + stratified_z + the torch.cat of rendering._sample_passes."""
    name = "sun_ray_table"
    R, G = _need(name, u, "u", F32, ("R", "G")).shape
    _need(name, rays, "rays", F32, (R, ">=6"))
    _need(name, d1, "d1", F32, R)
    K = _need(name, sun, "sun", F32, ("K", 3)).shape[0]
    table = _out(name, table, "table", F32, (K * R, 8), u.device, torch.empty)
    z_sun = _out(name, z_sun, "z_sun", F32, (K * R, G), u.device, torch.empty)
    _on_device(name, u, rays, d1, sun, table, z_sun)
    L.check(L.lib().bn_sun_ray_table(_p(rays), rays.shape[1], _p(d1), _p(sun), _p(u), R, K, G, _p(table), _p(z_sun), _stream()),
            "bn_sun_ray_table")
    return table, z_sun


def sun_shade_dirs(desc, sigma_sun, z_sun, rays_d, sun, acc=None, wsum=None, X=None, w=None, noise=None, noise_std=0.0, rgb=None,
                   vis=None, want_vis=False):
    """Transmittance of the sun pass and the shading that reads it, K directions in one launch (bn_sun_shade_dirs), forward only.
    sigma_sun, z_sun (K, R, G) (any shape of K R G elements in that order); noise (R, G) or None; either acc (R, C), wsum (R,) - one
    BRDF per ray - or X (R, G, C), w (R, G) - per-sample shading; rays_d (R, 3) view with unit inner stride; sun (K, 3).  rgb (K, R, 3)
    / vis (K, R): float32 on the device, rows contiguous - the planes may be further apart (a (K, i:j) slice of a whole view).
    -> rgb (K, R, 3) and vis (K, R) = T_{G-1} or None (with `vis` given or want_vis)."""
    name = "sun_shade_dirs"
    K = _need(name, sun, "sun", F32, ("K", 3)).shape[0]
    src = acc if acc is not None else X
    _need(name, sigma_sun, "sigma_sun", F32)
    R = src.shape[0] if isinstance(src, torch.Tensor) and src.dim() else sigma_sun.numel() // max(1, K)
    G = sigma_sun.numel() // max(1, K * R)
    dev = sigma_sun.device
    _need(name, sigma_sun, "sigma_sun", F32, K * R * G)
    _need(name, z_sun, "z_sun", F32, K * R * G)
    _maybe(name, noise, "noise", F32, (R, G))
    _maybe(name, acc, "acc", F32, (R, int(desc.C)))
    (_maybe if acc is None else _need)(name, wsum, "wsum", F32, R)                     # acc needs its wsum, X its w
    _maybe(name, X, "X", F32, (R, G, int(desc.C)))
    (_maybe if X is None else _need)(name, w, "w", F32, (R, G))
    rays_d = _need(name, rays_d, "rays_d", F32, (R, 3), "rows")
    if rgb is None:
        rgb = torch.empty((K, R, 3), dtype=torch.float32, device=dev)
    if vis is None and want_vis:
        vis = torch.empty((K, R), dtype=torch.float32, device=dev)
    if not plane_rows(_need(name, rgb, "rgb", F32, (K, R, 3), False)):
        raise ValueError(f"{name}: rgb with strides {rgb.stride()}: its (R, 3) planes must be contiguous rows that do not overlap")
    if _maybe(name, vis, "vis", F32, (K, R), False) is not None and (R > 1 and vis.stride(1) != 1 or K > 1 and vis.stride(0) < R):
        raise ValueError(f"{name}: vis with strides {vis.stride()}: its rows must be contiguous and must not overlap")
    _on_device(name, sigma_sun, z_sun, sun, acc, wsum, X, w, noise, rays_d, rgb, vis)
    rdp, rds = _rows3(rays_d, R)
    raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L.check(L.lib().bn_sun_shade_dirs(C.byref(desc), _p(sigma_sun), _p(z_sun), _p(noise), float(noise_std), _p(acc), _p(wsum), _p(X),
                                      _p(w), rdp, rds, _p(sun), R, G, K, raw(rgb), 3 * R if K == 1 else rgb.stride(0), raw(vis),
                                      R if (vis is None or K == 1) else vis.stride(0), _stream()), "bn_sun_shade_dirs")
    return rgb, vis


def sample_brdf(desc, X, rays, n1, S1, S2, out, backward_of=None, sun_col=8):
    """Per-sample BRDF of --MultiBRDF on stored field-output rows (bn_sample_brdf_forward / _backward).  X (N, C) rows of which the
    first n1 are S1 per ray and the rest S2 per ray; rays (R, >= 6) fp32 rows (sun at sun_col, < 0: ones).  Forward: `out` (N, 4) or
    (N, C) receives [bp, sigma(, the channels behind)].  backward_of = dB (N, 4 | C): `out` (N, C) receives d loss / d X."""
    N, Cc = X.shape
    assert X.is_cuda and X.dtype == torch.float32 and X.is_contiguous() and rays.dtype == torch.float32 and rays.stride(1) == 1
    assert out.is_contiguous() and out.dtype == torch.float32 and out.shape[0] == N
    R = rays.shape[0]
    assert n1 == R * S1 and (n1 == N or N - n1 == R * S2), (N, n1, R, S1, S2)
    if backward_of is None:
        L.check(L.lib().bn_sample_brdf_forward(C.byref(desc), _p(X), _p(rays), R, rays.stride(0), sun_col, N, n1, S1, S2, _p(out),
                                               out.shape[1], _stream()), "bn_sample_brdf_forward")
    else:
        dB = backward_of
        assert dB.is_contiguous() and dB.dtype == torch.float32 and dB.shape[0] == N and out.shape[1] == Cc
        L.check(L.lib().bn_sample_brdf_backward(C.byref(desc), _p(X), _p(rays), R, rays.stride(0), sun_col, N, n1, S1, S2, _p(dB),
                                                dB.shape[1], _p(out), _stream()), "bn_sample_brdf_backward")
    return out


def lambert_tail(z_all, idx, out1, out2, rgbs, rgb_padding, lambda_rgb, d_out1, d_out2, valid_depth=None, target_depth=None,
                 target_weight=None, target_std=None, lambda_ds=0.0, usealldepth=False, ray_loss=None, loss_acc=None, rgb=None,
                 weights=None, depth=None, nonfinite=None, noise=None):
    """Ray-level tail of a Lambertian step in one launch (bn_lambert_tail): merged compositing + shading + SNerfLoss +
    DepthLoss + the backward of all of it, gradient rows written to d_out1 / d_out2.  nonfinite ([2] int64 counters): rays with a
    non-finite loss term are left out and counted, non-finite gradient elements zeroed and counted."""
    R, S2 = z_all.shape
    S1, Cc = out1.shape[1], out1.shape[2]
    use = target_depth is not None and lambda_ds > 0
    dt = _depth_targets(use, valid_depth, target_depth, target_weight, target_std)
    L.check(L.lib().bn_lambert_tail(_p(z_all), _p(idx), _p(out1), _p(out2), S1, S2, Cc, R, _p(rgbs), *dt,
                                    float(rgb_padding), float(lambda_rgb), float(lambda_ds if use else 0.0),
                                    int(bool(usealldepth)), _p(ray_loss), _p(loss_acc), 0 if loss_acc is None else loss_acc.numel(),
                                    _p(rgb), _p(weights), _p(depth),
                                    _p(d_out1), _p(d_out2), _p(nonfinite), _nz(noise), _stream()), "bn_lambert_tail")


def adam_multi(param, grad, exp_avg, exp_avg_sq, groups, active, state, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
               grad_scale=1.0, zero_grad=True):
    """Adam over the (lo, hi) groups of one flat buffer in one launch; step counts / lr / draw counter from `state`."""
    n = len(groups)
    lo = (C.c_int64 * n)(*[g[0] for g in groups])
    hi = (C.c_int64 * n)(*[g[1] for g in groups])
    act = (C.c_int32 * n)(*[int(bool(a)) for a in active])
    L.check(L.lib().bn_adam_multi(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, lo, hi, act, float(betas[0]), float(betas[1]),
                                  float(eps), float(weight_decay), float(grad_scale), int(bool(zero_grad)), _p(state), _stream()),
            "bn_adam_multi")


# ----------------------------------------------------------------------------------------- BRDFs
def _opt(t):
    return None if t is None else _f32(t)


class RPVFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, l, v, n, w, k, theta, rhoc):
        l, v, n, w, k, theta, rhoc = [_opt(t) for t in (l, v, n, w, k, theta, rhoc)]
        N = n.shape[0]
        brdf = torch.empty(N, 3, dtype=torch.float32, device=n.device)
        aux = torch.empty(N, L.BN_BRDF_AUX, dtype=torch.float32, device=n.device)
        L.check(L.lib().bn_brdf_rpv_forward(_p(l), _p(v), _p(n), _p(w), _p(k), _p(theta), _p(rhoc), N, _p(brdf), _p(aux),
                                            _stream()), "bn_brdf_rpv_forward")
        ctx.save_for_backward(*[t if t is not None else torch.empty(0, device=n.device) for t in (l, v, n, w, k, theta, rhoc)])
        ctx.has = (k is not None, theta is not None, rhoc is not None)
        ctx.mark_non_differentiable(aux)
        return brdf, aux

    @staticmethod
    def backward(ctx, d_brdf, _d_aux):
        l, v, n, w, k, theta, rhoc = ctx.saved_tensors
        hk, ht, hr = ctx.has
        k, theta, rhoc = (k if hk else None), (theta if ht else None), (rhoc if hr else None)
        N = n.shape[0]
        mk = lambda on: torch.empty(N, 3, dtype=torch.float32, device=n.device) if on else None
        d_n, d_w, d_k, d_t, d_r = mk(True), mk(True), mk(hk), mk(ht), mk(hr)
        d_brdf = _f32(d_brdf)      # referenced until the launch is issued
        L.check(L.lib().bn_brdf_rpv_backward(_p(l), _p(v), _p(n), _p(w), _p(k), _p(theta), _p(rhoc), _p(d_brdf), N,
                                             _p(d_n), _p(d_w), _p(d_k), _p(d_t), _p(d_r), _stream()), "bn_brdf_rpv_backward")
        return None, None, d_n, d_w, d_k, d_t, d_r


class HapkeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, l, v, n, w, b, c, theta, hpk_scl, shell):
        l, v, n, w, b, c, theta = [_opt(t) for t in (l, v, n, w, b, c, theta)]
        N = n.shape[0]
        brdf = torch.empty(N, 3, dtype=torch.float32, device=n.device)
        aux = torch.empty(N, L.BN_BRDF_AUX, dtype=torch.float32, device=n.device)
        L.check(L.lib().bn_brdf_hapke_forward(_p(l), _p(v), _p(n), _p(w), _p(b), _p(c), _p(theta), float(hpk_scl), int(shell),
                                              N, _p(brdf), _p(aux), _stream()), "bn_brdf_hapke_forward")
        ctx.save_for_backward(*[t if t is not None else torch.empty(0, device=n.device) for t in (l, v, n, w, b, c, theta)])
        ctx.has = (b is not None, c is not None, theta is not None)
        ctx.hpk_scl, ctx.shell = float(hpk_scl), int(shell)
        ctx.mark_non_differentiable(aux)
        return brdf, aux

    @staticmethod
    def backward(ctx, d_brdf, _d_aux):
        l, v, n, w, b, c, theta = ctx.saved_tensors
        hb, hc, ht = ctx.has
        b, c, theta = (b if hb else None), (c if hc else None), (theta if ht else None)
        N = n.shape[0]
        mk = lambda on: torch.empty(N, 3, dtype=torch.float32, device=n.device) if on else None
        d_n, d_w, d_b, d_c = mk(True), mk(True), mk(hb), mk(hc)
        d_t = torch.empty(N, dtype=torch.float32, device=n.device) if ht else None
        d_brdf = _f32(d_brdf)      # referenced until the launch is issued
        L.check(L.lib().bn_brdf_hapke_backward(_p(l), _p(v), _p(n), _p(w), _p(b), _p(c), _p(theta), ctx.hpk_scl, ctx.shell,
                                               _p(d_brdf), N, _p(d_n), _p(d_w), _p(d_b), _p(d_c), _p(d_t), _stream()),
                "bn_brdf_hapke_backward")
        return None, None, d_n, d_w, d_b, d_c, d_t, None, None


class MicrofacetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, l, v, n, albedo, rough, f0):
        ctx.rough_shape = rough.shape
        l, v, n, albedo, rough = [_f32(t) for t in (l, v, n, albedo, rough.reshape(-1))]
        N = n.shape[0]
        brdf = torch.empty(N, 3, dtype=torch.float32, device=n.device)
        aux = torch.empty(N, L.BN_BRDF_AUX, dtype=torch.float32, device=n.device)
        L.check(L.lib().bn_brdf_microfacet_forward(_p(l), _p(v), _p(n), _p(albedo), _p(rough), float(f0), N, _p(brdf), _p(aux),
                                                   _stream()), "bn_brdf_microfacet_forward")
        ctx.save_for_backward(l, v, n, albedo, rough)
        ctx.f0 = float(f0)
        ctx.mark_non_differentiable(aux)
        return brdf, aux

    @staticmethod
    def backward(ctx, d_brdf, _d_aux):
        l, v, n, albedo, rough = ctx.saved_tensors
        N = n.shape[0]
        d_n = torch.empty(N, 3, dtype=torch.float32, device=n.device)
        d_a = torch.empty_like(d_n)
        d_r = torch.empty(N, dtype=torch.float32, device=n.device)
        d_brdf = _f32(d_brdf)      # referenced until the launch is issued
        L.check(L.lib().bn_brdf_microfacet_backward(_p(l), _p(v), _p(n), _p(albedo), _p(rough), ctx.f0, _p(d_brdf), N,
                                                    _p(d_n), _p(d_a), _p(d_r), _stream()), "bn_brdf_microfacet_backward")
        return None, None, d_n, d_a, d_r.reshape(ctx.rough_shape), None


# ----------------------------------------------------------------------------------------- optimizer
def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    L.check(L.lib().bn_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(lr), float(betas[0]),
                                 float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale), _stream()),
            "bn_adam_step")


# ----------------------------------------------------------------------------------------- debug
def count_nonfinite(x, counts=None):
    """check_nan without the host round trip (train_utils.py:14-25): adds the number of NaN / Inf elements of `x` to
    counts[0] / counts[1] (int64 device tensor, created zeroed when None) on the current stream and returns it."""
    x = _f32(x)
    if counts is None:
        counts = torch.zeros(2, dtype=torch.int64, device=x.device)
    if x.numel():
        L.check(L.lib().bn_count_nonfinite(_p(x), x.numel(), _p(counts), _stream()), "bn_count_nonfinite")
    return counts


# ------------------------------------------------------------------------------ the orthophoto entries
def _zone(name, zone, south):
    """(zone, south) as the entries take them: an integer zone from 1 to 60 (numpy integers included), south 0 or 1."""
    try:
        z = int(zone)
    except (TypeError, ValueError):
        z = 0
    if isinstance(zone, bool) or z != zone or not 1 <= z <= 60:
        raise ValueError(f"{name}: zone {zone!r} is not an integer from 1 to 60")
    return z, int(bool(south))


def utm_geodetic(en, zone, south, skipped):
    """Geodetic points of UTM points (bn_utm_geodetic): en (n, 2) float64 = (east, north) in `zone` -> lonlat (n, 2) float64 in
    degrees, NaN where a point is refused; skipped (1,) int64 on the device, accumulated into."""
    name = "utm_geodetic"
    en = _need(name, en, "en", F64, ("n", 2), "copy", cells=(0, 1 << 30))
    _need(name, skipped, "skipped", I64, 1)
    zone, south = _zone(name, zone, south)
    _on_device(name, en, skipped)
    n = en.shape[0]
    lonlat = torch.empty((n, 2), dtype=torch.float64, device=en.device)
    if n:
        with torch.cuda.device(en.device):
            L.check(L.lib().bn_utm_geodetic(_p(en), n, zone, south, _p(lonlat), _p(skipped), _stream()), "bn_utm_geodetic")
    return lonlat


def grid_pixels(rpc, dsm, xoff, yoff, res, zone, south, rows=None, colrow=None, counts=None):
    """The pixel of an image that every cell of a height grid projects to (bn_grid_pixels): rpc a camera.Rpc, dsm (H, W) float32
    with its Grid's origin and resolution, in the UTM `zone`.  rows = (row0, row1): only those rows are written (the others are
    uninitialised unless `colrow` comes in) and counted.  -> colrow (H, W, 2) float64 = (col, row), NaN where a cell is counted,
    counts (1,) int64, accumulated into when given."""
    name = "grid_pixels"
    _need(name, dsm, **VIS_DSM)
    zone, south = _zone(name, zone, south)
    xoff, yoff, res = float(xoff), float(yoff), float(res)
    if not (res > 0 and math.isfinite(res) and math.isfinite(xoff) and math.isfinite(yoff)):
        raise ValueError(f"{name}: origin ({xoff}, {yoff}) must be finite and resolution {res} positive and finite")
    H, W = dsm.shape
    row0, row1 = _rows(name, H, rows)
    colrow = _out(name, colrow, "colrow", F64, (H, W, 2), dsm.device, torch.empty)
    counts = _out(name, counts, "counts", I64, (1,), dsm.device, flat=True)
    _on_device(name, dsm, colrow, counts)
    with torch.cuda.device(dsm.device):
        L.check(L.lib().bn_grid_pixels(rpc.ref(), _p(dsm), H, W, xoff, yoff, res, row0, row1, zone, south, _p(colrow), _p(counts), _stream()),
                "bn_grid_pixels")
    return colrow, counts


GATHER_MODES = {"bilinear": L.BN_GATHER_BILINEAR, "nearest": L.BN_GATHER_NEAREST}


def image_gather(img, Hi, Wi, C_, strides, colrow, vis=None, cells=None, mode="bilinear", out=None, state=None, counts=None):
    """An image gathered at the pixels of n cells (bn_image_gather).  img: a contiguous float32 device buffer read through the
    element strides (row, col, channel) - no copy; colrow (..., 2) float64 = (col, row) per cell, vis uint8 per cell or None
    (only BN_VIS_VISIBLE cells are kept); cells = (n0, n1): only those cells are written (the others are uninitialised unless
    `out` / `state` come in) and counted.  -> out (C, n) float32, state (n,) uint8 in {0 no data, 1 outside, 2 occluded, 3 kept},
    counts (4,) int64, accumulated into when given."""
    name = "image_gather"
    Hi, Wi, C_ = int(Hi), int(Wi), int(C_)
    if mode not in GATHER_MODES:
        raise ValueError(f"{name}: mode {mode!r} ('bilinear' or 'nearest')")
    if Hi < 1 or Wi < 1 or not 1 <= C_ <= L.BN_GATHER_MAX_CHANNELS:
        raise ValueError(f"{name}: an image of {Hi} x {Wi} pixels and {C_} channels (at least 1 x 1, 1 to {L.BN_GATHER_MAX_CHANNELS} channels)")
    _need(name, img, "image", F32)
    sr, sc, sp = (int(s) for s in strides)
    last = (Hi - 1) * sr + (Wi - 1) * sc + (C_ - 1) * sp
    if min(sr, sc, sp) < 0 or last >= img.numel():
        raise ValueError(f"{name}: image of {img.numel()} elements is read through the strides {(sr, sc, sp)} up to element {last}")
    _need(name, colrow, "colrow", F64)
    if colrow.dim() < 1 or colrow.shape[-1] != 2 or colrow.numel() > 1 << 31:
        raise ValueError(f"{name}: colrow {tuple(colrow.shape)} is not (..., 2) with at most 2^30 cells")
    n = colrow.numel() // 2
    _maybe(name, vis, "vis", U8, n)
    n0, n1 = (0, n) if cells is None else (int(cells[0]), int(cells[1]))
    if not 0 <= n0 <= n1 <= n:
        raise ValueError(f"{name}: cells ({n0}, {n1}) outside [0, {n}]")
    out = _out(name, out, "out", F32, (C_, n), colrow.device, torch.empty, flat=True)
    state = _out(name, state, "state", U8, (n,), colrow.device, torch.empty, flat=True)
    counts = _out(name, counts, "counts", I64, (4,), colrow.device, flat=True)
    _on_device(name, img, colrow, vis, out, state, counts)
    with torch.cuda.device(colrow.device):
        L.check(L.lib().bn_image_gather(_p(img), Hi, Wi, C_, sr, sc, sp, _p(colrow), _p(vis), n0, n1, GATHER_MODES[mode], _p(out), n,
                                        _p(state), _p(counts), _stream()), "bn_image_gather")
    return out, state, counts


MOSAIC_MAPS = ("best", "best_val", "mean", "std")


def grid_mosaic(views, C_, dsm, xoff, yoff, res, zone, south, rows=None, mode="bilinear", colrow=None, count=None, best=None,
                best_val=None, mean=None, std=None, counts=None, sums=None, want=MOSAIC_MAPS):
    """The cells of a height grid under K images in one launch (bn_grid_mosaic).  views: K tuples (img, Hi, Wi, strides, vis, rank,
    rpc) - img a contiguous float32 device buffer of C_ channels read through the element strides (row, col, channel), as
    image_gather reads it; vis (H, W) uint8 of grid_visibility towards that view, or None; rank an integer, the smaller wins
    `best`; rpc a camera.Rpc.  dsm (H, W) float32 with its Grid's origin and resolution, in the UTM `zone`; colrow (K, H, W, 2)
    float64 or None: the views' pixels as grid_pixels gives them, used in place of the projection.  rows = (row0, row1): only
    those rows are written (the others are uninitialised unless the outputs come in) and counted.  count (H, W) uint8, best (H, W)
    int32, best_val / mean / std (C_, H, W) float32, counts (K, 5) int64 and sums (3,) int64 = (cells, q, skipped) may be given -
    counts and sums are accumulated into; a map that is neither given nor named in `want` is not computed (None).
    -> {"count", "best", "best_val", "mean", "std", "counts", "sums"}."""
    name = "grid_mosaic"
    K, C_, zone, south, (xoff, yoff, res), (H, W), (row0, row1), specs, held = _views_on_grid(name, views, C_, dsm, xoff, yoff, res, zone,
                                                                                          south, rows, mode)
    _maybe(name, colrow, "colrow", F64, (K, H, W, 2))
    dev = dsm.device
    wanted = lambda t, key: t is not None or key in want
    count = _out(name, count, "count", U8, (H, W), dev, torch.empty)
    best = _out(name, best, "best", I32, (H, W), dev, torch.empty) if wanted(best, "best") else None
    best_val = _out(name, best_val, "best_val", F32, (C_, H, W), dev, torch.empty) if wanted(best_val, "best_val") else None
    mean = _out(name, mean, "mean", F32, (C_, H, W), dev, torch.empty) if wanted(mean, "mean") else None
    std = _out(name, std, "std", F32, (C_, H, W), dev, torch.empty) if wanted(std, "std") else None
    counts = _out(name, counts, "counts", I64, (K, 5), dev)
    sums = _out(name, sums, "sums", I64, (3,), dev, flat=True)
    _on_device(name, dsm, colrow, count, best, best_val, mean, std, counts, sums, *held)
    table = _view_table(specs)
    with torch.cuda.device(dev):
        # the same bytes on the device, which the kernel reads; the library checks the host copy and copies nothing.  The copy and
        # the launch are on one stream, so the buffer may go back to the allocator when this call returns
        table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=U8).to(dev)
        L.check(L.lib().bn_grid_mosaic(table, _p(table_dev), K, C_, _p(dsm), H, W, xoff, yoff, res, row0, row1, zone, south,
                                       GATHER_MODES[mode], _p(colrow), _p(count), _p(best), _p(best_val), _p(mean), _p(std),
                                       _p(counts), _p(sums), _stream()), "bn_grid_mosaic")
    return {"count": count, "best": best, "best_val": best_val, "mean": mean, "std": std, "counts": counts, "sums": sums}


def _views_on_grid(name, views, C_, dsm, xoff, yoff, res, zone, south, rows, mode):
    """The host-side checks grid_mosaic and grid_sweep share: K views of C_ channels over the grid of `dsm`, each (img, Hi, Wi,
    strides, vis, rank, rpc) -> K, C_, zone, south, (xoff, yoff, res), (H, W), (row0, row1), the views' records for _view_table and
    the tensors they hold (for _on_device), or ValueError by `name`."""
    views = list(views)
    K, C_ = len(views), int(C_)
    if not 1 <= K <= L.BN_MOSAIC_MAX_VIEWS:
        raise ValueError(f"{name}: {K} views (1 to {L.BN_MOSAIC_MAX_VIEWS})")
    if not 1 <= C_ <= L.BN_MOSAIC_MAX_CHANNELS:
        raise ValueError(f"{name}: {C_} channels (1 to {L.BN_MOSAIC_MAX_CHANNELS})")
    if mode not in GATHER_MODES:
        raise ValueError(f"{name}: mode {mode!r} ('bilinear' or 'nearest')")
    _need(name, dsm, **VIS_DSM)
    zone, south = _zone(name, zone, south)
    xoff, yoff, res = float(xoff), float(yoff), float(res)
    if not (res > 0 and math.isfinite(res) and math.isfinite(xoff) and math.isfinite(yoff)):
        raise ValueError(f"{name}: origin ({xoff}, {yoff}) must be finite and resolution {res} positive and finite")
    H, W = dsm.shape
    row0, row1 = _rows(name, H, rows)
    held, specs = [], []
    for k, (img, Hi, Wi, strides, vis, rank, rpc) in enumerate(views):
        Hi, Wi = int(Hi), int(Wi)
        _need(name, img, f"image {k}", F32)
        sr, sc, sp = (int(s) for s in strides)
        last = (Hi - 1) * sr + (Wi - 1) * sc + (C_ - 1) * sp
        if Hi < 1 or Wi < 1 or min(sr, sc, sp) < 0 or last >= img.numel():
            raise ValueError(f"{name}: image {k} of {img.numel()} elements is read as {Hi} x {Wi} pixels through the strides "
                             f"{(sr, sc, sp)} up to element {last}")
        _maybe(name, vis, f"vis {k}", U8, (H, W))
        if isinstance(rank, bool) or int(rank) != rank or not -(1 << 31) <= int(rank) < 1 << 31:
            raise ValueError(f"{name}: rank {rank!r} of view {k} is not a 32-bit integer")
        held += [img, vis]
        specs.append((img, vis, Hi, Wi, sr, sc, sp, int(rank), rpc.struct))
    return K, C_, zone, south, (xoff, yoff, res), (H, W), (row0, row1), specs, held


def _view_table(specs):
    """_views_on_grid's records as the bn_mosaic_view table in host memory."""
    table = (L.MosaicView * len(specs))()
    for v, (img, vis, *scalars, rpc) in zip(table, specs):
        v.img, v.vis = img.data_ptr(), None if vis is None else vis.data_ptr()
        v.Hi, v.Wi, v.s_row, v.s_col, v.s_chan, v.rank = scalars
        v.rpc = rpc
    return table


def _sweep_offsets(name, offsets):
    """Z offsets in metres, a sequence or a tensor of any real dtype -> (Z,) float64 on the HOST (the entry checks them there), Z in
    [1, BN_SWEEP_MAX_LEVELS], every one finite, or ValueError by name."""
    try:
        off = torch.as_tensor(offsets).detach().to(device="cpu", dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name}: offsets {offsets!r} are not a sequence of numbers") from None
    if off.dim() != 1 or not 1 <= off.numel() <= L.BN_SWEEP_MAX_LEVELS:
        raise ValueError(f"{name}: offsets {tuple(off.shape)} are not 1 to {L.BN_SWEEP_MAX_LEVELS} levels")
    if not bool(torch.isfinite(off).all()):
        raise ValueError(f"{name}: every offset must be finite")
    return off.contiguous()


def _sweep_min_views(name, min_views):
    """The views a level needs to be valid: an integer (not a bool) from 1 to BN_MOSAIC_MAX_VIEWS -> int, or ValueError by name."""
    if isinstance(min_views, bool) or not isinstance(min_views, numbers.Integral) or not 1 <= min_views <= L.BN_MOSAIC_MAX_VIEWS:
        raise ValueError(f"{name}: min_views {min_views!r} is not an integer from 1 to {L.BN_MOSAIC_MAX_VIEWS}")
    return int(min_views)


def grid_sweep(views, C_, dsm, xoff, yoff, res, zone, south, offsets, min_views=2, rows=None, mode="bilinear", colrow=None, level=None,
               cost_min=None, count=None, altitude=None, cost=None, valid=None, wins=None, sums=None, want_cost=False):
    """The altitude sweep of a height grid under K images in one launch (bn_grid_sweep).  views, C_, dsm, xoff, yoff, res, zone, south,
    rows, mode: as grid_mosaic takes them (a view's rank is not read).  offsets: Z floats in metres, 1 to 256, any order; min_views:
    a level needs that many views to be valid.  colrow (Z, K, H, W, 2) float64 or None: the pixels per level and view, used in place
    of the projection.  level (H, W) int32, cost_min and altitude (H, W) float32, count (H, W) uint8, cost (Z, H, W) float32 (made only
    with want_cost, or given), valid and wins (Z,) int64 and sums (3,) int64 = (cells, q, skipped) may be given - the counters are
    accumulated into.  -> {"level", "cost_min", "count", "altitude", "cost" or None, "valid", "wins", "sums", "offsets" (Z,) float64 on
    the host}."""
    name = "grid_sweep"
    K, C_, zone, south, (xoff, yoff, res), (H, W), (row0, row1), specs, held = _views_on_grid(name, views, C_, dsm, xoff, yoff, res, zone,
                                                                                          south, rows, mode)
    off = _sweep_offsets(name, offsets)
    Z = off.numel()
    min_views = _sweep_min_views(name, min_views)
    _maybe(name, colrow, "colrow", F64, (Z, K, H, W, 2))
    dev = dsm.device
    level = _out(name, level, "level", I32, (H, W), dev, torch.empty)
    cost_min = _out(name, cost_min, "cost_min", F32, (H, W), dev, torch.empty)
    count = _out(name, count, "count", U8, (H, W), dev, torch.empty)
    altitude = _out(name, altitude, "altitude", F32, (H, W), dev, torch.empty)
    if cost is not None or want_cost:
        cost = _out(name, cost, "cost", F32, (Z, H, W), dev, torch.empty)
    valid = _out(name, valid, "valid", I64, (Z,), dev, flat=True)
    wins = _out(name, wins, "wins", I64, (Z,), dev, flat=True)
    sums = _out(name, sums, "sums", I64, (3,), dev, flat=True)
    _on_device(name, dsm, colrow, level, cost_min, count, altitude, cost, valid, wins, sums, *held)
    table = _view_table(specs)
    with torch.cuda.device(dev):
        # the table and the offsets twice, as grid_mosaic passes its table: the library checks the host copies and copies nothing
        table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=U8).to(dev)
        off_dev = off.to(dev)
        L.check(L.lib().bn_grid_sweep(table, _p(table_dev), K, C_, _p(dsm), H, W, xoff, yoff, res, row0, row1, zone, south,
                                      GATHER_MODES[mode], off.numpy().ctypes.data_as(C.POINTER(C.c_double)), _p(off_dev), Z, min_views,
                                      _p(colrow), _p(level), _p(cost_min), _p(count), _p(altitude), _p(cost), _p(valid), _p(wins),
                                      _p(sums), _stream()), "bn_grid_sweep")
    return {"level": level, "cost_min": cost_min, "count": count, "altitude": altitude, "cost": cost, "valid": valid, "wins": wins,
            "sums": sums, "offsets": off}


AGG_VOLUME = dict(shape=("H", "W", "Z"), side=(1, (1 << 31) - 1), cells=(1, (1 << 31) - 1))   # [H][W][Z] int32 of the aggregation entries


def _agg_volume(name, t, what):
    """quanta or sum: int32 [H][W][Z] with Z in [1, BN_SWEEP_MAX_LEVELS] and fewer than 2^31 elements -> H, W, Z."""
    _need(name, t, what, I32, **AGG_VOLUME)
    if t.shape[2] > L.BN_SWEEP_MAX_LEVELS:
        raise ValueError(f"{name}: {what} {tuple(t.shape)} has more than {L.BN_SWEEP_MAX_LEVELS} levels")
    return tuple(t.shape)


def cost_quanta(cost, quantum, quanta=None, counters=None):
    """A cost volume as integer quanta (bn_cost_quanta).  cost (Z, H, W) float32, NaN where a level is not valid at a cell; quantum > 0:
    the cost of one quantum.  quanta (H, W, Z) int32 and counters (3,) int64 = (cells with a result, valid pairs, capped pairs) may be
    given - the counters are accumulated into.  -> quanta, counters."""
    name = "cost_quanta"
    _need(name, cost, "cost", F32, ("Z", "H", "W"), side=(1, (1 << 31) - 1), cells=(1, (1 << 31) - 1))
    Z, H, W = cost.shape
    if Z > L.BN_SWEEP_MAX_LEVELS:
        raise ValueError(f"{name}: cost {tuple(cost.shape)} has more than {L.BN_SWEEP_MAX_LEVELS} levels")
    if isinstance(quantum, bool) or not isinstance(quantum, numbers.Real) or not (math.isfinite(quantum) and quantum > 0):
        raise ValueError(f"{name}: quantum {quantum!r} must be finite and positive")
    quanta = _out(name, quanta, "quanta", I32, (H, W, Z), cost.device, torch.empty)
    counters = _out(name, counters, "counters", I64, (3,), cost.device, flat=True)
    _on_device(name, cost, quanta, counters)
    with torch.cuda.device(cost.device):
        L.check(L.lib().bn_cost_quanta(_p(cost), Z, H, W, float(quantum), _p(quanta), _p(counters), _stream()), "bn_cost_quanta")
    return quanta, counters


def _agg_penalties(name, P1, P2):
    """The penalties in quanta: integers (not bools) with 0 <= P1 <= P2 <= 2^20, or ValueError by name."""
    for v in (P1, P2):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{name}: penalties P1={P1!r}, P2={P2!r} must be integers")
    if not 0 <= P1 <= P2 <= L.BN_AGG_QINV:
        raise ValueError(f"{name}: penalties P1={P1}, P2={P2} (0 <= P1 <= P2 <= {L.BN_AGG_QINV})")
    return int(P1), int(P2)


def cost_paths(quanta, P1, P2, mask=0xFF, sum=None):
    """The minimum-cost paths of the directions in `mask` (bits 0 to 7, include/brdfnerf_hip.h) ADDED into sum (bn_cost_paths).
    quanta (H, W, Z) int32 as cost_quanta gives them; P1 <= P2: the penalties in quanta; sum (H, W, Z) int32, zeroed when made here.
    -> sum."""
    name = "cost_paths"
    H, W, Z = _agg_volume(name, quanta, "quanta")
    P1, P2 = _agg_penalties(name, P1, P2)
    if isinstance(mask, bool) or not isinstance(mask, numbers.Integral) or not 1 <= mask <= 0xFF:
        raise ValueError(f"{name}: direction mask {mask!r} (bits 0 to 7, at least one)")
    sum = _out(name, sum, "sum", I32, (H, W, Z), quanta.device)
    _on_device(name, quanta, sum)
    with torch.cuda.device(quanta.device):
        L.check(L.lib().bn_cost_paths(_p(quanta), Z, H, W, P1, P2, int(mask), _p(sum), _stream()), "bn_cost_paths")
    return sum


def cost_pick(quanta, sum, level=None, sum_min=None, wins=None, sums=None):
    """The first valid level of the smallest sum per cell (bn_cost_pick).  quanta, sum (H, W, Z) int32; level, sum_min (H, W) int32,
    wins (Z,) int64 and sums (2,) int64 = (cells, the sum of sum_min) may be given - the counters are accumulated into.
    -> {"level", "sum_min", "wins", "sums"}."""
    name = "cost_pick"
    H, W, Z = _agg_volume(name, quanta, "quanta")
    _need(name, sum, "sum", I32, (H, W, Z))
    dev = quanta.device
    level = _out(name, level, "level", I32, (H, W), dev, torch.empty)
    sum_min = _out(name, sum_min, "sum_min", I32, (H, W), dev, torch.empty)
    wins = _out(name, wins, "wins", I64, (Z,), dev, flat=True)
    sums = _out(name, sums, "sums", I64, (2,), dev, flat=True)
    _on_device(name, quanta, sum, level, sum_min, wins, sums)
    with torch.cuda.device(dev):
        L.check(L.lib().bn_cost_pick(_p(quanta), _p(sum), Z, H, W, _p(level), _p(sum_min), _p(wins), _p(sums), _stream()), "bn_cost_pick")
    return {"level": level, "sum_min": sum_min, "wins": wins, "sums": sums}


def _cast_scalars(name, center, rng, xoff, yoff, res, zmax):
    center = tuple(float(v) for v in center)
    rng, xoff, yoff, res, zmax = float(rng), float(xoff), float(yoff), float(res), float(zmax)
    if len(center) != 3 or not all(math.isfinite(v) for v in center):
        raise ValueError(f"{name}: centre {center} must be 3 finite numbers")
    if not (rng > 0 and math.isfinite(rng)):
        raise ValueError(f"{name}: range {rng} must be positive and finite")
    if not (res > 0 and math.isfinite(res)):
        raise ValueError(f"{name}: resolution {res} must be positive and finite")
    if not (math.isfinite(xoff) and math.isfinite(yoff)):
        raise ValueError(f"{name}: grid origin ({xoff}, {yoff}) is not finite")
    if math.isnan(zmax):
        raise ValueError(f"{name}: zmax is NaN")
    return center, rng, xoff, yoff, res, zmax


def cast_rays(rays, center, rng, dsm, xoff, yoff, res, zmax=float("inf"), depth=None, state=None, cell=None, nan_cells=None,
              counts=None, want_cell=True, want_nan=True):
    """The depth at which rays meet a height grid (bn_cast_rays): rays (R, >= 8) float32 rows with unit inner stride (o, d, near,
    far), center (3 floats) and rng the normalisation of a UTM scene, dsm (H, W) float32 with its Grid's origin and resolution.
    depth (R,) float32, state (R,) uint8, cell (R,) int32, nan_cells (R,) int32 and counts (5,) int64 may be given - slices of a
    view's buffers, say - and counts are accumulated into; cell / nan_cells are made unless want_cell / want_nan say otherwise.
    -> depth, state, cell or None, nan_cells or None, counts."""
    name = "cast_rays"
    rays = _need(name, rays, "rays", F32, ("R", ">=8"), "rows")
    _need(name, dsm, **VIS_DSM)
    center, rng, xoff, yoff, res, zmax = _cast_scalars(name, center, rng, xoff, yoff, res, zmax)
    R = rays.shape[0]
    if R > (1 << 30):
        raise ValueError(f"{name}: {R} rays (0 to 2^30)")
    if R > 1 and rays.stride(0) < 8:
        rays = rays.contiguous()
    H, W = dsm.shape
    dev = dsm.device
    depth = _out(name, depth, "depth", F32, (R,), dev, torch.empty)
    state = _out(name, state, "state", U8, (R,), dev, torch.empty)
    if cell is not None or want_cell:
        cell = _out(name, cell, "cell", I32, (R,), dev, torch.empty)
    if nan_cells is not None or want_nan:
        nan_cells = _out(name, nan_cells, "nan_cells", I32, (R,), dev, torch.empty)
    counts = _out(name, counts, "counts", I64, (5,), dev)
    _on_device(name, rays, dsm, depth, state, cell, nan_cells, counts)
    if R:
        with torch.cuda.device(dev):
            L.check(L.lib().bn_cast_rays(C.c_void_p(rays.data_ptr()), rays.stride(0) if R > 1 else rays.shape[1], R,
                                         (C.c_double * 3)(*center), rng, _p(dsm), H, W, xoff, yoff, res, zmax, _p(depth), _p(state),
                                         _p(cell), _p(nan_cells), _p(counts), _stream()), "bn_cast_rays")
    return depth, state, cell, nan_cells, counts


def _horizon_az(name, az):
    """(D, 2) or (2,) azimuths (east, north) in any float dtype -> (D, 2) float64 on the HOST (the entries check them there), D in
    [1, BN_HORIZON_MAX_DIRS], every component finite and no row (0, 0), or ValueError by name."""
    az = torch.as_tensor(az)
    if not az.is_floating_point():
        raise ValueError(f"{name}: az are {az.dtype}, not a float dtype")
    az = az.detach().to(device="cpu", dtype=torch.float64)
    if az.dim() == 1 and az.numel() == 2:
        az = az.reshape(1, 2)
    if az.dim() != 2 or az.shape[1] != 2 or not 1 <= az.shape[0] <= L.BN_HORIZON_MAX_DIRS:
        raise ValueError(f"{name}: az {tuple(az.shape)} are not (D, 2) or (2,) with D from 1 to {L.BN_HORIZON_MAX_DIRS}")
    if not bool(torch.isfinite(az).all()) or not bool((az != 0).any(1).all()):
        raise ValueError(f"{name}: every azimuth must be finite and not (0, 0)")
    return az.contiguous()


def _horizon_scalars(name, res, max_steps, zmax):
    res, zmax = float(res), float(zmax)
    max_steps = (1 << 31) - 1 if max_steps is None else min(int(max_steps), (1 << 31) - 1)
    if not (res > 0 and math.isfinite(res)):
        raise ValueError(f"{name}: resolution {res} must be positive and finite")
    if max_steps < 1:
        raise ValueError(f"{name}: max_steps {max_steps} must be at least 1")
    if math.isnan(zmax):
        raise ValueError(f"{name}: zmax is NaN")
    return res, max_steps, zmax


def grid_horizon(dsm, res, az, max_steps=None, zmax=float("inf"), rows=None, slope=None, hit=None, want_hit=False):
    """The horizon of the cells of a height grid (bn_grid_horizon): dsm (H, W) float32 on the device, az (D, 2) (east, north)
    horizontal vectors, taken to float64 on the host.  max_steps bounds the march in cells along the dominant axis (None: the
    grid's longer side).  rows = (row0, row1): only those rows are written (the others are uninitialised unless `slope` / `hit`
    come in).  slope (D, H, W) float32 and hit (D, H, W) int32 may be given.  -> slope, hit or None (want_hit, or `hit` given)."""
    name = "grid_horizon"
    _need(name, dsm, **VIS_DSM)
    az = _horizon_az(name, az)
    res, max_steps, zmax = _horizon_scalars(name, res, max_steps, zmax)
    H, W = dsm.shape
    D = az.shape[0]
    row0, row1 = _rows(name, H, rows)
    slope = _out(name, slope, "slope", F32, (D, H, W), dsm.device, torch.empty)
    if hit is not None or want_hit:
        hit = _out(name, hit, "hit", I32, (D, H, W), dsm.device, torch.empty)
    _on_device(name, dsm, slope, hit)
    with torch.cuda.device(dsm.device):
        L.check(L.lib().bn_grid_horizon(_p(dsm), H, W, res, row0, row1, az.numpy().ctypes.data_as(C.POINTER(C.c_double)), D, max_steps,
                                        zmax, _p(slope), _p(hit), _stream()), "bn_grid_horizon")
    return slope, hit


def points_horizon(points, dsm, xoff, yoff, res, az, max_steps=None, zmax=float("inf"), want_hit=False):
    """The horizon of world points over a height grid (bn_points_horizon): points (R, 3) float64 (east, north, altitude) on the
    device (point_cloud's output), dsm (H, W) float32 with its Grid's origin and resolution, az (D, 2).
    -> slope (D, R) float32, hit (D, R) int32 or None."""
    name = "points_horizon"
    points = _need(name, points, **VIS_POINTS)
    _need(name, dsm, **VIS_DSM)
    az = _horizon_az(name, az)
    res, max_steps, zmax = _horizon_scalars(name, res, max_steps, zmax)
    xoff, yoff = float(xoff), float(yoff)
    if not (math.isfinite(xoff) and math.isfinite(yoff)):
        raise ValueError(f"{name}: grid origin ({xoff}, {yoff}) is not finite")
    _on_device(name, points, dsm)
    H, W = dsm.shape
    R, D = points.shape[0], az.shape[0]
    slope = torch.empty((D, R), dtype=torch.float32, device=dsm.device)
    hit = torch.empty((D, R), dtype=torch.int32, device=dsm.device) if want_hit else None
    if R:
        with torch.cuda.device(dsm.device):
            L.check(L.lib().bn_points_horizon(_p(points), R, _p(dsm), H, W, xoff, yoff, res, az.numpy().ctypes.data_as(C.POINTER(C.c_double)),
                                              D, max_steps, zmax, _p(slope), _p(hit), _stream()), "bn_points_horizon")
    return slope, hit


def sky_view(slope, acc, D, cells=None, svf=None, sums=None, last=True):
    """One tile of the sky-view sum (bn_sky_view): slope (n, ...) float32 planes of the horizon entries, acc float64 with one
    element per start, zeroed by the caller before the first tile and accumulated into, plane by plane in ascending order; D the
    TOTAL number of azimuths.  cells = (c0, c1): only those starts (flat indices) are read and written.  last=True (the tile of the
    last planes): svf (float32, acc's shape) = acc / D and sums (3,) int64 += (sum of llrint(svf 2^30) over the non-NaN ones, their
    count, the NaN count); svf and sums may be given - sums are accumulated into.  -> acc, svf or None, sums or None."""
    name = "sky_view"
    _need(name, slope, "slope", F32, None)
    _need(name, acc, "acc", F64, None)
    n_cells = acc.numel()
    if slope.dim() < 1 or not 1 <= slope.shape[0] <= L.BN_HORIZON_MAX_DIRS or n_cells < 1 or slope.numel() != slope.shape[0] * n_cells:
        raise ValueError(f"{name}: slope {tuple(slope.shape)} is not 1 to {L.BN_HORIZON_MAX_DIRS} planes of acc's {n_cells} elements")
    if n_cells > (1 << 30):
        raise ValueError(f"{name}: acc {tuple(acc.shape)} (1 to 2^30 elements)")
    D = int(D)
    if not 1 <= D <= L.BN_HORIZON_MAX_DIRS:
        raise ValueError(f"{name}: D {D} outside [1, {L.BN_HORIZON_MAX_DIRS}]")
    c0, c1 = (0, n_cells) if cells is None else (int(cells[0]), int(cells[1]))
    if not 0 <= c0 <= c1 <= n_cells:
        raise ValueError(f"{name}: cells ({c0}, {c1}) outside [0, {n_cells}]")
    if last:
        svf = _out(name, svf, "svf", F32, tuple(acc.shape), acc.device, torch.empty)
        sums = _out(name, sums, "sums", I64, (3,), acc.device)
    elif svf is not None or sums is not None:
        raise ValueError(f"{name}: svf and sums belong to the last tile (last=True)")
    _on_device(name, slope, acc, svf, sums)
    with torch.cuda.device(acc.device):
        L.check(L.lib().bn_sky_view(_p(slope), slope.shape[0], n_cells, c0, c1, _p(acc), D, _p(svf), _p(sums), _stream()), "bn_sky_view")
    return acc, svf, sums
