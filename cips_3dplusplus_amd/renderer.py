"""FiLM-SIREN volume renderer modules (parameter containers + the fused HIP render call).

Class names, constructor arguments, parameter names/shapes and initialisation follow
/root/reference/exp/cips3d/volume_renderer.py:15-190 so that a reference `state_dict` loads
unchanged (`renderer.sigmoid_beta`, `renderer.network.pts_linears.{i}.{weight,bias,gamma.*,beta.*}`,
`views_linears.*`, `rgb_linear.*`, `sigma_linear.*`).  The arithmetic itself lives in
csrc/nerf.hip: `VolumeFeatureRenderer.render` launches linear_table (FiLM heads) -> nerf_render ->
nerf_finish; per-point activations never reach HBM.
"""
import math

import torch
from torch import nn

from . import hip


def _uniform(shape, bound):
    return torch.empty(*shape).uniform_(-bound, bound)


class LinearLayer(nn.Module):
    """volume_renderer.py:15-35: out = std_init * (x W^T + b) + bias_init (constants applied at run time)."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, std_init=1, freq_init=False, is_first=False):
        super().__init__()
        if is_first:
            w = _uniform((out_dim, in_dim), 1 / in_dim)
        elif freq_init:
            w = _uniform((out_dim, in_dim), math.sqrt(6 / in_dim) / 25)
        else:
            w = 0.25 * nn.init.kaiming_normal_(torch.randn(out_dim, in_dim), a=0.2, mode="fan_in",
                                               nonlinearity="leaky_relu")
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(_uniform((out_dim,), math.sqrt(1 / in_dim)))
        self.bias_init = bias_init
        self.std_init = std_init

    def forward(self, input):
        if input.numel() // input.shape[-1] > 64:       # point tensors (b, ..., n, c): MFMA path
            return hip.points_linear(input, self.weight, self.bias, out_scale=float(self.std_init),
                                     out_shift=float(self.bias_init))
        x = input.reshape(-1, input.shape[-1]).contiguous()
        y = hip.linear(x, self.weight, self.bias, out_scale=float(self.std_init), out_shift=float(self.bias_init))
        return y.view(*input.shape[:-1], -1)


class FiLMSiren(nn.Module):
    """volume_renderer.py:39-85: sin(gamma(style) * (x W^T + b) + beta(style))."""

    def __init__(self, in_channel, out_channel, style_dim, is_first=False):
        super().__init__()
        self.in_channel, self.out_channel = in_channel, out_channel
        bound = 1 / 3 if is_first else math.sqrt(6 / in_channel) / 25
        self.weight = nn.Parameter(_uniform((out_channel, in_channel), bound))
        self.bias = nn.Parameter(_uniform((out_channel,), math.sqrt(1 / in_channel)))
        self.gamma = LinearLayer(style_dim, out_channel, bias_init=30, std_init=15)
        self.beta = LinearLayer(style_dim, out_channel, bias_init=0, std_init=0.25)

    @torch.no_grad()
    def forward(self, input, style):
        """volume_renderer.py:70-85: input (b, ..., in), style (b, style_dim) -> sin(gamma * (x W^T + b) + beta).
        (The generator itself never materialises per-point activations: csrc/nerf.hip fuses all layers.)"""
        film = torch.stack([self.gamma(style), self.beta(style)], 1).contiguous()       # [B, 2, out]
        return hip.points_linear(input, self.weight, self.bias, film=film)


class SirenGenerator(nn.Module):
    """volume_renderer.py:89-116 (construction order matters for seeded init parity)."""

    def __init__(self, D=8, W=256, style_dim=256, input_ch=3, input_ch_views=3, output_features=True, **kwargs):
        super().__init__()
        self.D, self.W, self.style_dim = D, W, style_dim
        self.input_ch, self.input_ch_views, self.output_features = input_ch, input_ch_views, output_features
        self.pts_linears = nn.ModuleList([FiLMSiren(3, W, style_dim=style_dim, is_first=True)] +
                                         [FiLMSiren(W, W, style_dim=style_dim) for _ in range(D - 1)])
        self.views_linears = FiLMSiren(input_ch_views + W, W, style_dim=style_dim)
        self.rgb_linear = LinearLayer(W, 3, freq_init=True)
        self.sigma_linear = LinearLayer(W, 1, freq_init=True)

    @torch.no_grad()
    def points_forward(self, x, styles):
        """volume_renderer.py:133-160: x (b, ..., n, 3 + 3) = [normalised points, view dirs], styles (b, D+1, style_dim)
        -> rgb (.., 3), sdf (.., 1), features (.., W), all per point (layer by layer, materialised)."""
        pts, views = torch.split(x, [self.input_ch, self.input_ch_views], dim=-1)
        h = pts.contiguous()
        for i, layer in enumerate(self.pts_linears):
            h = layer(h, styles[:, i])
        sdf = self.sigma_linear(h)
        feat = self.views_linears(torch.cat([h, views], -1), styles[:, -1])
        return self.rgb_linear(feat), sdf, feat

    def forward(self, x, styles, forward_points=None):
        return self.points_forward(x=x, styles=styles)


class VolumeFeatureRenderer(nn.Module):
    """volume_renderer.py:163-190 container; `render` is the fused replacement of
    prepare_nerf_inputs + forward + volume_integration (nerf_utils.py:173-338, volume_renderer.py:192-303)."""

    def __init__(self, N_layers_renderer, input_dim, hidden_dim, style_dim, view_dim, with_sdf, output_features,
                 **kwargs):
        super().__init__()
        if input_dim != 3 or view_dim != 3:
            raise NotImplementedError("the HIP renderer implements input_dim=3, view_dim=3")
        self.N_layers_renderer = N_layers_renderer
        self.input_dim, self.hidden_dim, self.style_dim, self.view_dim = input_dim, hidden_dim, style_dim, view_dim
        self.with_sdf, self.output_features = with_sdf, output_features
        self.sigmoid_beta = nn.Parameter(0.1 * torch.ones(1))
        self.network = SirenGenerator(D=N_layers_renderer, W=hidden_dim, style_dim=style_dim, input_ch=input_dim,
                                      input_ch_views=view_dim, output_features=output_features)
        # Built on first use, on whichever stream calls first, and read from every stream a forward is issued on (pipeline.py's
        # lanes): each entry carries a hip.BuildFence, and every accessor below orders the calling stream behind the build once.
        self._derived = None      # (key, packed, layer_bias, fence)
        self._packed_t = None     # (transposed stream, fence)
        self._packed32 = None     # (key, exact-fp32 weight stream, fence): built on first use in "fp32_exact" precision
        self._packed32_t = None   # (key, exact-fp32 stream of the transposed matrices, fence): the eikonal loss's reverse sweep
        self.exact_fp32 = False
        self._tables = {}         # B -> (styles_buf, film_buf, LinearTable)

    # ---- derived, weight-dependent device buffers (re-made when a parameter changes) ------------
    def _weights_key(self):
        # (the parameter list is cached: walking the module tree is most of what this key costs per forward)
        ent = self.__dict__.get("_wk_params")
        w0 = self.network.views_linears._parameters["weight"]
        if ent is None or ent[0] is not w0:
            net = self.network
            ps = [l.weight for l in net.pts_linears] + [l.bias for l in net.pts_linears] + \
                 [net.views_linears.weight, net.views_linears.bias]
            ent = self.__dict__["_wk_params"] = (w0, ps)
        return tuple((p.data_ptr(), p._version) for p in ent[1])

    def set_precision(self, precision):
        """"fp32" (default): the point MLP's GEMMs as fp32-equivalent split-fp16 products (three exact fp16 products per fp32
        product, fp32 accumulate: csrc/nerf.hip); "fp32_exact": the fp32 matrix instruction on fp32 operands -- IEEE fp32
        products, the arithmetic of the reference's F.linear (cips3d/volume_renderer.py:15-35, 74-85) -- through
        the F32 instantiation of the same kernel (hidden_dim 256, inference; ~2.3x the render time)."""
        if precision not in ("fp32", "fp32_exact"):
            raise ValueError(precision)
        if precision == "fp32_exact" and self.hidden_dim != 256:
            raise NotImplementedError("the exact-fp32 render kernel is built for hidden_dim = 256")
        self.exact_fp32 = precision == "fp32_exact"
        return self

    def packed32(self, force=False):
        """The exact-fp32 weight stream (None in the default precision), re-made when a weight changes.  force: build it in
        any precision (the SDF gradient kernel always multiplies on the fp32 matrix instruction)."""
        if not self.exact_fp32 and not force:
            return None
        key = self._weights_key()
        if self._packed32 is None or self._packed32[0] != key:
            net = self.network
            D, H = self.N_layers_renderer, self.hidden_dim
            with torch.no_grad():
                w_hidden = torch.stack([l.weight for l in net.pts_linears[1:]]).contiguous() if D > 1 else None
                p32 = hip.nerf_pack_weights32(w_hidden, net.views_linears.weight.detach().contiguous(), H, D)
            self._packed32 = (key, p32, hip.BuildFence(p32))
        self._packed32[2].wait()
        return self._packed32[1]

    def _derived_buffers(self):
        key = self._weights_key()
        if self._derived is None or self._derived[0] != key:
            net = self.network
            D, H = self.N_layers_renderer, self.hidden_dim
            with torch.no_grad():
                w_hidden = torch.stack([l.weight for l in net.pts_linears[1:]]).contiguous() if D > 1 else None
                packed = hip.nerf_pack_weights(w_hidden, net.views_linears.weight.detach().contiguous(), H, D)
                layer_bias = torch.stack([l.bias for l in net.pts_linears] + [net.views_linears.bias]).contiguous()
            self._derived = (key, packed, layer_bias, hip.BuildFence(packed, layer_bias))
            self._packed_t = None
        self._derived[3].wait()
        return self._derived[1], self._derived[2]

    def _packed_transposed(self):
        """The transposed weight stream of the fused backward, made on first use (inversion only)."""
        packed, _ = self._derived_buffers()
        if self._packed_t is None:
            net = self.network
            D, H = self.N_layers_renderer, self.hidden_dim
            with torch.no_grad():
                w_hidden = torch.stack([l.weight for l in net.pts_linears[1:]]).contiguous() if D > 1 else None
                pt = hip.nerf_pack_weights_t(w_hidden, net.views_linears.weight.detach().contiguous(), packed, H, D)
            self._packed_t = (pt, hip.BuildFence(pt))
        self._packed_t[1].wait()
        return self._packed_t[0]

    def _film_table(self, B, device, lane=0):
        net = self.network
        key = (B, net.views_linears.gamma.weight.data_ptr())
        slot = B if lane == 0 else (B, lane)
        ent = self._tables.get(slot)
        if ent is None or ent[0] != key:
            D, H, S = self.N_layers_renderer, self.hidden_dim, self.style_dim
            styles_buf = torch.empty(B, D + 1, S, device=device)
            film = torch.empty(B, D + 1, 2, H, device=device)
            tab = hip.LinearTable(device, lane)
            layers = list(net.pts_linears) + [net.views_linears]
            for l, layer in enumerate(layers):
                for j, head in enumerate((layer.gamma, layer.beta)):
                    tab.add(head.weight, head.bias, styles_buf, (D + 1) * S, film, (D + 1) * 2 * H,
                            out_scale=float(head.std_init), out_shift=float(head.bias_init),
                            x_offset=l * S, out_offset=(l * 2 + j) * H)
            ent = (key, styles_buf, film, tab)
            self._tables[slot] = ent
        return ent[1], ent[2], ent[3]

    @torch.no_grad()
    def render(self, cam_poses, focals, near, far, styles, img_size, N_samples, perturb_u=None,
               static_viewdirs=False, return_sdf=False, n_chunks=None, film=None, stash=None, zero_words=None, planar_mask=False):
        """cam_poses (B,3,4), focals/near/far (B,1,1), styles (B,D+1,style_dim)
        -> thumb_rgb (B,3,S,S), features (B,H,S,S), sdf (B,S,S,N,1)|None, mask (B,2,S,S), xyz (B,3,S,S)
        zero_words: a float32 scratch tensor the launch leaves zeroed (cips3d_nerf_params.zero_words).
        planar_mask: mask comes back as (2,B,S,S) -- the layout Generator.forward splits into its `mask` and `depth` maps."""
        B = cam_poses.shape[0]
        dev = cam_poses.device
        D, H = self.N_layers_renderer, self.hidden_dim
        net = self.network
        packed, layer_bias = self._derived_buffers()
        if film is None:
            styles_buf, film, tab = self._film_table(B, dev)
            styles_buf.copy_(styles)
            tab.run(B)
        else:                       # FiLM table computed by the caller (differentiable path: autograd.film_table)
            film = film.detach().float().contiguous()
        if stash is not None:       # differentiable forward: hip.nerf_forward_stash buffers, filled for the fused backward
            if self.exact_fp32:
                # the stash instantiation and the fused backward exist in split-fp16 arithmetic only: gradients would be taken
                # against another forward than the one inference runs in this mode
                raise NotImplementedError('set_precision("fp32_exact") is inference-only: the differentiable forward (stash + fused '
                                          'backward) has no exact-fp32 instantiation; use set_precision("fp32") for gradients')
            n_chunks = stash["n_chunks"]
        if n_chunks is None:
            n_chunks = hip.nerf_suggest_chunks(B, img_size, N_samples)
        R = img_size * img_size
        sdf = torch.empty(B, R, N_samples, device=dev) if return_sdf else None
        features, thumb, xyz, mask = hip.nerf_render_maps(cam_poses=cam_poses.float().contiguous(), focals=focals.float().reshape(B).contiguous(),
                        near_=near.float().reshape(B).contiguous(), far_=far.float().reshape(B).contiguous(),
                        perturb_u=None if perturb_u is None else perturb_u.float().reshape(B, R).contiguous(),
                        w_first=net.pts_linears[0].weight, packed=packed, w_view=net.views_linears.weight, film=film,
                        layer_bias=layer_bias, w_sigma=net.sigma_linear.weight, w_rgb=net.rgb_linear.weight,
                        b_sigma=net.sigma_linear.bias, b_rgb=net.rgb_linear.bias, sigmoid_beta=self.sigmoid_beta,
                        B=B, img_size=img_size, n_samples=N_samples, hidden=H, depth=D,
                        static_viewdirs=int(bool(static_viewdirs)), n_chunks=n_chunks, sdf=sdf,
                        raw_density=not self.with_sdf, packed32=None if stash is not None else self.packed32(),
                        stash=None if stash is None else stash["stash"], bwd_sdf=None if stash is None else stash["sdf"],
                        bwd_crgb=None if stash is None else stash["crgb"], zero_words=zero_words, planar_mask=planar_mask)
        if sdf is not None:
            sdf = sdf.view(B, img_size, img_size, N_samples, 1)
        return thumb, features, sdf, mask, xyz

    def _sdf_grad(self, film, near, far, B, N, **geom):
        """hip.nerf_sdf_grad with this renderer's weights and the FiLM table `film` [B, D+1, 2, H]."""
        D, H = self.N_layers_renderer, self.hidden_dim
        if not hip.nerf_sdf_grad_supported(H, D):
            raise NotImplementedError(f"the SDF gradient (eikonal term) kernel is built for hidden_dim = 256 and depth <= 64; this "
                                      f"renderer has hidden_dim = {H}, depth = {D}")
        net = self.network
        _, layer_bias = self._derived_buffers()
        return hip.nerf_sdf_grad(near_=near.float().reshape(B).contiguous(), far_=far.float().reshape(B).contiguous(),
                                 w_first=net.pts_linears[0].weight, packed32=self.packed32(force=True) if D > 1 else None,
                                 film=film, layer_bias=layer_bias, w_sigma=net.sigma_linear.weight, b_sigma=net.sigma_linear.bias,
                                 B=B, n_samples=N, hidden=H, depth=D, **geom)

    @torch.no_grad()
    def sdf_gradient(self, cam_poses, focals, near, far, styles, img_size, N_samples, perturb_u=None, static_viewdirs=False,
                     film=None):
        """d sdf / d pts at the sample points `render` evaluates for the same arguments (the reference's `eikonal_term`,
        nerf_utils.py:221-228: autograd.grad(sdf, pts, ones) with pts the un-normalised world points) -> sdf (B,S,S,N,1),
        grad (B,S,S,N,3).  One forward-mode pass through the FiLM-SIREN trunk on the exact-fp32 matrix instruction
        (csrc/nerf_sdf_grad.hip), whatever `set_precision` says; the view layer is not part of it, so `static_viewdirs` does not
        change the result.  styles (B, D+1, style_dim), or `film`: a FiLM table [B, D+1, 2, H] computed by the caller (styles
        is then not read).  No autograd graph: the result is a constant.

        Runs on the caller's stream through the renderer's lane-0 FiLM table: do not issue it from inside a `ViewPipeline` lane
        (pipeline.py) while that pipeline has views in flight."""
        if not self.with_sdf:
            raise NotImplementedError("with_sdf=False: the network's output is a raw density, not a distance (the reference "
                                      "computes the eikonal term only in its SDF branch)")
        if not hip.nerf_sdf_grad_supported(self.hidden_dim, self.N_layers_renderer):
            raise NotImplementedError(f"sdf_gradient: the kernel is built for hidden_dim = 256 and depth <= 64; this renderer has "
                                      f"hidden_dim = {self.hidden_dim}, depth = {self.N_layers_renderer}")
        B, dev = cam_poses.shape[0], cam_poses.device
        if film is None:
            styles_buf, film, tab = self._film_table(B, dev)
            styles_buf.copy_(styles)
            tab.run(B)
        else:
            film = film.detach().float().contiguous()
        R = img_size * img_size
        sdf, grad = self._sdf_grad(film, near, far, B, N_samples, img_size=img_size, cam_poses=cam_poses.float().contiguous(),
                                   focals=focals.float().reshape(B).contiguous(),
                                   perturb_u=None if perturb_u is None else perturb_u.float().reshape(B, R).contiguous())
        return sdf.view(B, img_size, img_size, N_samples, 1), grad.view(B, img_size, img_size, N_samples, 3)

    def packed32_t(self):
        """The exact-fp32 stream of the TRANSPOSED hidden matrices in reverse layer order (cips3d_nerf_eikonal_loss's packed32_t:
        the reverse sweep multiplies by W_l^T for l = D-1 .. 1), cached beside `packed32` and re-made when a weight changes."""
        key = self._weights_key()
        ent = self._packed32_t
        if ent is None or ent[0] != key:
            net = self.network
            D, H = self.N_layers_renderer, self.hidden_dim
            with torch.no_grad():
                w_t = torch.stack([l.weight.t() for l in reversed(net.pts_linears[1:])]).contiguous() if D > 1 else None
                p32 = hip.nerf_pack_weights32(w_t, net.views_linears.weight.detach().contiguous(), H, D)
            ent = self._packed32_t = (key, p32, hip.BuildFence(p32))
        ent[2].wait()
        return ent[1]

    def _eikonal_refusals(self, what):
        if not self.with_sdf:
            raise NotImplementedError(f"{what}: with_sdf=False: the network's output is a raw density, not a distance (the reference "
                                      "applies the eikonal and minimal-surface terms only in its SDF branch)")
        if not hip.nerf_eikonal_supported(self.hidden_dim, self.N_layers_renderer):
            raise NotImplementedError(f"{what}: the kernel is built for hidden_dim = 256 and depth <= 64; this renderer has "
                                      f"hidden_dim = {self.hidden_dim}, depth = {self.N_layers_renderer}")

    def _eikonal_args(self, near, far, B, N, **geom):
        """film -> the keyword arguments of hip.nerf_eikonal_loss for this renderer's weights (autograd.EikonalLossFn's `call`)."""
        D, H = self.N_layers_renderer, self.hidden_dim
        net = self.network
        _, layer_bias = self._derived_buffers()
        fixed = dict(near_=near.detach().float().reshape(B).contiguous(), far_=far.detach().float().reshape(B).contiguous(),
                     w_first=net.pts_linears[0].weight.detach(), packed32=self.packed32(force=True) if D > 1 else None,
                     packed32_t=self.packed32_t() if D > 1 else None, layer_bias=layer_bias, w_sigma=net.sigma_linear.weight.detach(),
                     b_sigma=net.sigma_linear.bias.detach(), B=B, n_samples=N, hidden=H, depth=D, **geom)
        return lambda film: dict(fixed, film=film)

    def _film_torch(self, styles, B):
        """The FiLM table [B, D+1, 2, H] in torch ops (LinearLayer: std_init (s W^T + b) + bias_init), differentiable."""
        F = torch.nn.functional
        net = self.network
        if styles.shape[0] != B:
            styles = styles.expand(B, -1, -1)
        rows = []
        for l, layer in enumerate(list(net.pts_linears) + [net.views_linears]):
            st = styles[:, l]
            gb = [float(h.std_init) * F.linear(st, h.weight.detach().to(st.dtype), h.bias.detach().to(st.dtype)) + float(h.bias_init)
                  for h in (layer.gamma, layer.beta)]
            rows.append(torch.stack(gb, 1))
        return torch.stack(rows, 1)

    def _eikonal_torch(self, film, pts, near, far, beta):
        """The two losses as a torch expression (the reference's: autograd.grad(sdf, pts, create_graph=True), then
        exp/stylesdf/losses.py:13-24) of the table `film` and the world points pts [B, P, 3]: the A/B partner of the kernel."""
        F = torch.nn.functional
        net = self.network
        dt = film.dtype
        B = pts.shape[0]
        with torch.enable_grad():
            p = pts.detach().to(dt).clone().requires_grad_(True)
            h = p * 2 / (far.detach().to(dt) - near.detach().to(dt)).reshape(B, 1, 1)
            for l, layer in enumerate(net.pts_linears):
                pre = F.linear(h, layer.weight.detach().to(dt), layer.bias.detach().to(dt))
                h = torch.sin(film[:, l, 0].unsqueeze(1) * pre + film[:, l, 1].unsqueeze(1))
            sdf = F.linear(h, net.sigma_linear.weight.detach().to(dt), net.sigma_linear.bias.detach().to(dt))
            g, = torch.autograd.grad(sdf, p, torch.ones_like(sdf), create_graph=True)
            eik = ((g.norm(dim=-1) - 1) ** 2).mean()
            ms = torch.exp(-beta * sdf.abs()).mean()
        return eik, ms

    @staticmethod
    def _camera_points(cam_poses, focals, near, far, img_size, N_samples, perturb_u, dt):
        """The world sample points [B, S*S*N, 3] of `render` for a camera, in torch ops (nerf_utils.py:18-66, 69-121 offset
        sampling, 136-170), constants."""
        with torch.no_grad():
            B, S, N = cam_poses.shape[0], int(img_size), int(N_samples)
            dev = cam_poses.device
            c2w, focal = cam_poses.to(dt), focals.to(dt).reshape(B, 1, 1)
            nr, fr = near.to(dt).reshape(B, 1, 1, 1), far.to(dt).reshape(B, 1, 1, 1)
            centres = torch.linspace(0.5, S - 0.5, S, dtype=dt, device=dev)
            y = centres.view(1, S, 1).expand(1, S, S)
            x = centres.view(1, 1, S).expand(1, S, S)
            d_cam = torch.stack([(x - S * 0.5) / focal, -(y - S * 0.5) / focal, -torch.ones(B, S, S, dtype=dt, device=dev)], dim=-1)
            rays_d = (d_cam.unsqueeze(-2) * c2w[:, None, None, :3, :3]).sum(-1)
            rays_o = c2w[:, None, None, :3, 3].expand_as(rays_d)
            t = torch.linspace(0.0, 1.0 - 1.0 / N, N, dtype=dt, device=dev).view(1, 1, 1, N)
            z = (nr * (1.0 - t) + fr * t).expand(B, S, S, N)
            if perturb_u is not None:
                upper = torch.cat([z[..., 1:], fr.expand(B, S, S, 1)], dim=-1)
                z = z + (upper - z) * perturb_u.to(dt).reshape(B, S, S, 1)
            pts = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z.unsqueeze(-1)
            return pts.reshape(B, S * S * N, 3)

    def eikonal_loss(self, cam_poses, focals, near, far, styles, img_size, N_samples, perturb_u=None, film=None, beta=100,
                     weights=None):
        """The reference's two SDF regularisers (exp/stylesdf/losses.py:13-24 on autograd.grad(sdf, pts, create_graph=True),
        nerf_utils.py:221-228) at the sample points `render` evaluates for the same arguments -> (eikonal, minimal_surface) =
        (mean((|d sdf / d pts| - 1)^2), mean(exp(-beta |sdf|))), two 0-dim fp32 tensors whose graph reaches `styles` through
        `autograd.film_table` (a [1, D+1, style_dim] latent is broadcast over the B views), or through `film`, a FiLM table
        [B, D+1, 2, H] the caller computed (styles is then not read).  One node (autograd.EikonalLossFn, csrc/nerf_eikonal.hip):
        forward-mode pass and reverse sweep in one kernel on the exact-fp32 matrix instruction; the renderer's own weights, the
        points and the camera are constants.  weights = (w_e, w_m): -> (w_e eikonal + w_m minimal_surface, eikonal,
        minimal_surface) with only the first differentiable -- one kernel call instead of two.
        With CIPS3D_FUSED_EIKONAL=0 in the environment, or on CPU tensors, the same losses are a torch expression with
        create_graph=True (the A/B partner; any float dtype of `styles` / `film`).
        Raises NotImplementedError for hidden_dim != 256 and for with_sdf=False.  The lane-0 note of `sdf_gradient` applies."""
        import os
        from . import autograd as AG
        self._eikonal_refusals("eikonal_loss")
        B, S, N = cam_poses.shape[0], int(img_size), int(N_samples)
        fused = cam_poses.is_cuda and os.environ.get("CIPS3D_FUSED_EIKONAL", "1") != "0"
        if not fused:
            if film is None:
                film = self._film_torch(styles, B)
            pts = self._camera_points(cam_poses, focals, near, far, S, N, perturb_u, film.dtype)
            eik, ms = self._eikonal_torch(film, pts, near, far, float(beta))
            if film.dtype == torch.float32:
                eik, ms = eik.float(), ms.float()
            return (eik, ms) if weights is None else (float(weights[0]) * eik + float(weights[1]) * ms, eik.detach(), ms.detach())
        if film is None:
            film = AG.film_table(self, styles, batch=B)
        R = S * S
        call = self._eikonal_args(near, far, B, N, img_size=S, cam_poses=cam_poses.detach().float().contiguous(),
                                  focals=focals.detach().float().reshape(B).contiguous(), beta=float(beta),
                                  perturb_u=None if perturb_u is None else perturb_u.detach().float().reshape(B, R).contiguous())
        return AG.EikonalLossFn.apply(film, call, weights)

    @torch.no_grad()
    def normal_map(self, cam_poses, focals, near, far, styles, img_size, N_samples, perturb_u=None, film=None, shade=None,
                   grad=None, sdf=None):
        """Composited surface normals of the view `render` produces for the same arguments: the render's compositing weights
        applied to d sdf / d pts (csrc/nerf_normals.hip) -> {"normal_raw": (B,3,S,S) = sum_i w_i grad_i, "normal": (B,3,S,S) =
        F.normalize(normal_raw) (zero where no sample has weight)}.  Runs `sdf_gradient` first unless its results are handed in
        (`sdf` (B,S,S,N[,1]) and `grad` (B,S,S,N,3), e.g. a forward's eikonal term); `styles` / `film` as there.
        shade = dict(light=(B,3), xyz=(B,3,S,S) the render's map[, eye=(B,3): default the camera position cam_poses[:, :, 3]]
        [, ka, kd, ks, shininess: default hip.PHONG_DEFAULTS][, u8_out: a contiguous uint8 (B,3,S,S) tensor to write into]) adds
        "shade" (B,1,S,S) fp32 and "shade_u8" (B,3,S,S) uint8: pytorch3d's Phong for a white surface, per pixel -- the picture the
        reference rasterises from the frame's depth mesh (render_video_web_v10.py:1839-1890), whose vertices are the pixels.
        The same refusals and the same lane-0 note as `sdf_gradient`."""
        if not self.with_sdf:
            raise NotImplementedError("with_sdf=False: the network's output is a raw density, not a distance: it has no surface "
                                      "normal (the reference computes the gradient only in its SDF branch)")
        if not hip.nerf_sdf_grad_supported(self.hidden_dim, self.N_layers_renderer):
            raise NotImplementedError(f"normal_map: the SDF gradient kernel is built for hidden_dim = 256 and depth <= 64; this "
                                      f"renderer has hidden_dim = {self.hidden_dim}, depth = {self.N_layers_renderer}")
        B, S, N = cam_poses.shape[0], int(img_size), int(N_samples)
        R = S * S
        if grad is None or sdf is None:
            sdf, grad = self.sdf_gradient(cam_poses, focals, near, far, styles, S, N, perturb_u=perturb_u, film=film)
        kw, want = {}, ("normal_raw", "normal")
        if shade is not None:
            unknown = set(shade) - {"light", "xyz", "eye", "ka", "kd", "ks", "shininess", "u8_out"}
            if unknown or "light" not in shade or "xyz" not in shade:
                raise ValueError(f"normal_map: shade needs light and xyz, and may hold eye, ka, kd, ks, shininess, u8_out; got "
                                 f"{sorted(shade)}")
            eye = shade.get("eye")
            eye = cam_poses[:, :, 3] if eye is None else eye
            kw = dict(xyz=shade["xyz"].float().reshape(B, 3, R).contiguous(), eye=eye.float().reshape(B, 3).contiguous(),
                      light=shade["light"].float().reshape(B, 3).contiguous(), shade_u8_out=shade.get("u8_out"),
                      **{k: shade[k] for k in ("ka", "kd", "ks", "shininess") if k in shade})
            want += ("shade", "shade_u8")
        out = hip.nerf_normals(sdf=sdf.float().reshape(B, R, N).contiguous(), grad=grad.float().reshape(B, R, N, 3).contiguous(),
                               sigmoid_beta=self.sigmoid_beta, B=B, n_samples=N, img_size=S,
                               cam_poses=cam_poses.float().contiguous(), focals=focals.float().reshape(B).contiguous(),
                               near_=near.float().reshape(B).contiguous(), far_=far.float().reshape(B).contiguous(),
                               perturb_u=None if perturb_u is None else perturb_u.float().reshape(B, R).contiguous(),
                               want=want, **kw)
        ret = {"normal": out["normal"].view(B, 3, S, S), "normal_raw": out["normal_raw"].view(B, 3, S, S)}
        if shade is not None:
            ret["shade"], ret["shade_u8"] = out["shade"].view(B, 1, S, S), out["shade_u8"].view(B, 3, S, S)
        return ret

    @torch.no_grad()
    def run_network(self, inputs, viewdirs, styles=None):
        """volume_renderer.py:282-303: per-point (rgb, sdf, features) for normalised points + per-ray view directions."""
        dirs = viewdirs.unsqueeze(-2).expand(inputs.shape)
        return self.network(torch.cat([inputs, dirs], -1), styles=styles)

    @torch.no_grad()
    def forward(self, pts, rays_d, viewdirs, z_vals, near, far, styles=None, return_eikonal=False, N_samples_forward=None,
                film=None, n_chunks=None):
        """The reference entry (volume_renderer.py:192-303): explicit sample points instead of a camera.
        pts (b h w N 3) or (b hw N 3); rays_d / viewdirs (b h w 3) | (b hw 3); z_vals (b h w N) | (b hw N); near / far
        (b 1 1); styles (b, D+1, style_dim) -> rgb_map (.., 3), feature_map (.., C), sdf (.., N, 1), mask (.., 2),
        xyz (.., 3), eikonal_term.  Runs the same fused kernel in its explicit-geometry instantiation;
        `N_samples_forward` (a memory bound of the reference) is accepted and ignored.
        film: a FiLM table [B, D+1, 2, H] computed by the caller (styles is then not read), n_chunks: the chunks a ray's samples
        are split into -- both as in `render`.
        return_eikonal: eikonal_term = d sdf / d pts, the shape of `pts` (volume_renderer.py:223-226), from the gradient kernel
        (`sdf_gradient`; a constant, no graph); None otherwise and for with_sdf=False renderers, as in the reference."""
        if return_eikonal and self.with_sdf and not hip.nerf_sdf_grad_supported(self.hidden_dim, self.N_layers_renderer):
            raise NotImplementedError(f"return_eikonal: the SDF gradient kernel is built for hidden_dim = 256 and depth <= 64; this "
                                      f"renderer has hidden_dim = {self.hidden_dim}, depth = {self.N_layers_renderer}")
        B = pts.shape[0]
        lead = pts.shape[:-2]
        N = pts.shape[-2]
        D, H = self.N_layers_renderer, self.hidden_dim
        dev = pts.device
        p = pts.float().reshape(B, -1, N, 3).contiguous()
        R = p.shape[1]
        d = rays_d.float().reshape(B, R, 3).contiguous()
        v = viewdirs.float().reshape(B, R, 3).contiguous()
        z = z_vals.float().reshape(B, R, N).contiguous()
        net = self.network
        packed, layer_bias = self._derived_buffers()
        if film is None:
            styles_buf, film, tab = self._film_table(B, dev)
            styles_buf.copy_(styles)
            tab.run(B)
        else:
            film = film.detach().float().contiguous()
        if n_chunks is None:
            n_chunks = max(1, min(N, hip.nerf_suggest_chunks(B, max(1, int(R ** 0.5)), N)))
        sdf = torch.empty(B, R, N, device=dev)
        features, thumb, xyz, mask = hip.nerf_render_maps(near_=near.float().reshape(B).contiguous(), far_=far.float().reshape(B).contiguous(),
                        w_first=net.pts_linears[0].weight, packed=packed, w_view=net.views_linears.weight, film=film,
                        layer_bias=layer_bias, w_sigma=net.sigma_linear.weight, w_rgb=net.rgb_linear.weight,
                        b_sigma=net.sigma_linear.bias, b_rgb=net.rgb_linear.bias, sigmoid_beta=self.sigmoid_beta,
                        B=B, img_size=1, n_samples=N, hidden=H, depth=D, static_viewdirs=0, n_chunks=n_chunks,
                        sdf=sdf, x_pts=p, x_rays_d=d, x_viewdirs=v, x_z_vals=z, n_rays=R, raw_density=not self.with_sdf,
                        packed32=self.packed32())
        eik = None
        if return_eikonal and self.with_sdf:
            eik = self._sdf_grad(film, near, far, B, N, x_pts=p, n_rays=R, want_sdf=False)[1].view(*lead, N, 3)
        to_rays = lambda t: t.view(B, t.shape[1], R).transpose(1, 2).reshape(*lead, t.shape[1]).contiguous()
        return to_rays(thumb), to_rays(features), sdf.view(*lead, N, 1), to_rays(mask), to_rays(xyz), eik
