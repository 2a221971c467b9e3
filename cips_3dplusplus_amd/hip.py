"""Thin tensor-level wrappers over the C ABI (one function per entry point of include/cips3d_hip.h).

PyTorch is used for device memory and streams only: outputs are allocated with torch, pointers and
the current stream are handed to the HIP library.  Nothing here computes on the host.
"""
import ctypes as C

import os

import torch

from . import _lib
from ._lib import dev_ptr, stream_ptr, check

MOD_DEMODULATE = 1
MOD_PACKED = 2
MOD_CHAINED = 4       # with MOD_PACKED: k-steps in the MFMA D-layout order (cips3d_fused_up_conv_next)
MOD_FLIP = 8          # with MOD_PACKED and ksq = 9: taps stored 180 degrees rotated (up-sampling branch of cips3d_modconv3x3)
MOD_SPLIT = 16        # with MOD_PACKED and ksq = 1: fp16 hi + lo fragments of 2^8 wm for the split-fp16 GEMM mode (GEMM_SPLIT)
MOD_SPLIT16 = 32      # with MOD_PACKED [| MOD_CHAINED]: split-fp16 fragments for the fused up-sampling stage (16-channel k-groups)
MOD_TRANSPOSE = 64    # with MOD_PACKED and ksq = 1 (fp32 fragments): the packed form of wm^T (data-gradient GEMM operand)
MOD_BF16 = 128        # with MOD_PACKED and ksq = 1: bf16 A fragments for modconv1x1_planes16 (bf16 decoder mode)

# bench.py sets this to a list to collect (start, end) event pairs around the dominant kernel's launch;
# events are recorded on the stream the kernel is launched on (torch's current stream).
KERNEL_EVENTS = {}
# An event record between two kernels drains the queue (~6 us bubble on MI355X), so a bench that times every launch slows
# the step it measures by 2-3 %: collect on every n-th call only, with event handles created ahead of the timed region.
KERNEL_EVENTS_STRIDE = 1
KERNEL_EVENTS_PHASE = 0      # the call within each stride that is timed (0 = the first; a bench picks a mid-region one)
_EVENT_POOL = []
_event_calls = {}


def prepare_event_pairs(n):
    """Create n (start, stop) event pairs with live hipEvent_t handles now (a handle only exists after a first record)."""
    for _ in range(n):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(); ev[1].record()
        _EVENT_POOL.append(ev)


def want_events(name):
    """The list to append this call's event pair to, or None (not collecting / not this call's turn)."""
    lst = KERNEL_EVENTS.get(name)
    if lst is None:
        return None
    k = _event_calls.get(name, 0)
    _event_calls[name] = k + 1
    st = max(1, KERNEL_EVENTS_STRIDE)
    return lst if k % st == KERNEL_EVENTS_PHASE % st else None


class DecoderMarks:
    """Timeline of the decoder launches of ONE cips3d_generator_forward call (cips3d_forward_io.ev_marks): hipEvent_t handles
    the call records before / after each decoder launch, and what each launch was.  Measurement only (bench.py); set
    `hip.DECODER_MARKS = DecoderMarks()` and the next Generator.forward fills it, then read `intervals()` after a
    synchronise."""
    KINDS = {0: "start", 1: "planes_gemm", 2: "gemm", 3: "lowres_gemm", 4: "fused_stage", 5: "torgb", 6: "other"}

    def __init__(self, n=40):
        self.events = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
        for e in self.events:
            e.record()                                # materialise the hipEvent_t handles
        self.handles = (C.c_void_p * n)(*[e.cuda_event for e in self.events])
        self.info = (C.c_int32 * (4 * n))()
        self.count = C.c_int32(0)
        self.n = n

    def io_fields(self):
        return (C.addressof(self.handles), C.addressof(self.info), C.addressof(self.count), self.n)

    def intervals(self):
        """[(kind, C_in, C_out, H_out, microseconds)] for launch k = mark k-1 -> mark k (after torch.cuda.synchronize()).
        fused_stage: C_in = the stage's width, C_out = the width of the next stage's low-resolution GEMM it also computes (0:
        none)."""
        out = []
        for k in range(1, self.count.value):
            out.append((self.KINDS.get(self.info[4 * k], "?"), self.info[4 * k + 1], self.info[4 * k + 2], self.info[4 * k + 3],
                        self.events[k - 1].elapsed_time(self.events[k]) * 1e3))
        return out


DECODER_MARKS = None      # a DecoderMarks: filled by the next one-call forward, then reset to None


def event_pair():
    if _EVENT_POOL:
        return _EVENT_POOL.pop()
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(); ev[1].record()              # materialise the hipEvent_t handles
    return ev


def _timed(name):
    lst = want_events(name)
    if lst is None:
        return None
    ev = event_pair()
    lst.append(ev)
    ev[0].record()
    return ev


def linear(x, W, bias=None, out=None, w_scale=1.0, b_scale=1.0, pixelnorm=False, lrelu=False, act_gain=1.0,
           out_scale=1.0, out_shift=0.0, trunc_mean=None, trunc_psi=1.0, out_repeat=1, out_repeat_stride=0):
    """x [B,in] -> [B,out]; see cips3d_linear."""
    lib = _lib.load()
    B, in_dim = x.shape
    out_dim = W.shape[0]
    if out is None:
        out = torch.empty(B, out_dim, device=x.device, dtype=torch.float32)
    if B == 0:           # (an empty tensor has no address to hand over; the entry point launches nothing for B = 0 either)
        return out
    check(lib.cips3d_linear(dev_ptr(x, "x"), x.stride(0), dev_ptr(W, "W"), dev_ptr(bias, "bias", True), dev_ptr(out, "out"),
                            out.stride(0), B, in_dim, out_dim, w_scale, b_scale, int(pixelnorm), int(lrelu), act_gain,
                            out_scale, out_shift, dev_ptr(trunc_mean, "trunc_mean", True), trunc_psi, out_repeat, out_repeat_stride,
                            stream_ptr()),
          "cips3d_linear")
    return out


# Bumped by everything that rewrites a module's style tables (FiLM table, decoder modulations: LinearTable.run, a full
# ForwardPlan.run): a forward plan's resident frame (plan.run, styles_resident) is only valid while nothing has since the plan's
# last full run, and checks that.  One counter per LANE: the tables of lane k > 0 are
# private to the forward plans of that lane (Generator.forward on another stream, pipeline.ViewPipeline).
import collections
STYLE_EPOCHS = collections.defaultdict(int)


class BuildFence:
    """Marks the point of the building stream at which device buffers that are built once and then read from several streams
    (the renderer's packed weight streams, the mean latents, a noise projector's meshes) are complete.  Made right after the
    build, on the stream that ran it; `wait()` on a reader's side orders the current stream behind that point the FIRST time
    the stream is seen, and is a set lookup afterwards.  `tensors` are marked as in use by every reading stream (allocator safety:
    a cache that drops them must not hand their memory out while another stream's kernels still read it).  No device: no-op."""
    __slots__ = ("event", "seen", "tensors")

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if torch.is_tensor(t) and t.is_cuda]
        self.event, self.seen = None, set()
        if torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
            self.event = torch.cuda.Event()
            self.event.record()
            self.seen.add(stream_ptr())

    def __reduce__(self):
        # (a copied or unpickled owner: events are not copied.  Its parameters live at new addresses, so the owner's cache key
        # no longer matches and the buffers are rebuilt with a fence of their own)
        return (BuildFence, ())

    def wait(self):
        if self.event is None:
            return
        sid = stream_ptr()
        if sid in self.seen:
            return
        if torch.cuda.is_current_stream_capturing():
            return              # (a capture cannot wait for work outside it: graphs run on lane 0's buffers, see Generator)
        cur = torch.cuda.current_stream()
        cur.wait_event(self.event)
        for t in self.tensors:
            t.record_stream(cur)
        self.seen.add(sid)


class StreamTail:
    """The end of the last piece of work that went through state shared by all streams (Generator's per-op forwards: the lane-0
    style tables).  `record()` marks the current stream's position, `wait()` orders the current stream behind the last mark when
    that was made on another stream.  One event, re-recorded: a wait refers to the record that preceded it."""
    __slots__ = ("event", "sid")

    def __init__(self):
        self.event, self.sid = None, None

    def __reduce__(self):
        return (StreamTail, ())

    def record(self):
        if not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
            return
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()
        self.sid = stream_ptr()

    def wait(self):
        if self.sid is None or self.sid == stream_ptr() or torch.cuda.is_current_stream_capturing():
            return
        torch.cuda.current_stream().wait_event(self.event)


class LinearTable:
    """A device-resident table of independent dense heads evaluated by one launch."""

    def __init__(self, device, lane=0):
        self.device = device
        self.lane = lane
        self._descs = []
        self._rows = 0
        self._dev = None
        self._keep = []

    def __deepcopy__(self, memo):
        # descriptors hold raw device pointers of the ORIGINAL module; the owners key their caches on parameter
        # addresses and rebuild the table for a copied module
        return LinearTable(self.device, self.lane)

    def add(self, W, bias, x, x_stride, out, out_stride, w_scale=1.0, b_scale=1.0, out_scale=1.0, out_shift=0.0,
            x_offset=0, out_offset=0):
        out_dim, in_dim = W.shape
        d = _lib.LinearDesc()
        d.W = dev_ptr(W, "W")
        d.bias = dev_ptr(bias, "bias", True)
        d.x = dev_ptr(x, "x") + 4 * x_offset
        d.out = dev_ptr(out, "out") + 4 * out_offset
        d.x_stride, d.out_stride = x_stride, out_stride
        d.in_dim, d.out_dim = in_dim, out_dim
        d.w_scale, d.b_scale, d.out_scale, d.out_shift = w_scale, b_scale, out_scale, out_shift
        d.row_begin = self._rows
        self._rows += out_dim
        self._descs.append(d)
        self._keep += [W, bias, x, out]
        self._dev = None

    def _upload(self):
        arr = (_lib.LinearDesc * len(self._descs))(*self._descs)
        raw = bytes(memoryview(arr))
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        self._dev = host.to(self.device)

    def repointed(self, x_base, x_tensor, x_stride=None):
        """This table with every head reading its input from `x_tensor` (a contiguous fp32 tensor laid out like the staging
        buffer whose base address is `x_base`) instead of from that buffer -- the caller's own W+ styles, without the copy launch
        into the staging buffer.  x_stride = 0: ONE row broadcast to every sample of the batch (a [1, ...] latent for B views; the
        backward's atomics then sum the batch's gradients into that row).  The uploaded descriptors are cached per (address,
        stride): a parameter that an optimiser updates in place keeps its address from step to step, so the steady state uploads
        nothing.  Returns None the first time an address is seen (a tensor that is new on every call would cost an upload per
        call -- more than the copy it saves): the caller then stages as before."""
        key = (x_tensor.data_ptr(), x_stride)
        cache = self.__dict__.setdefault("_repointed", {})
        ent = cache.get(key)
        if ent is None:
            seen, self.__dict__["_repoint_seen"] = self.__dict__.get("_repoint_seen"), key
            if seen != key:
                return None
            if len(cache) >= 4:
                cache.clear()
            ent = LinearTable(self.device, self.lane)
            for d in self._descs:
                c = _lib.LinearDesc.from_buffer_copy(d)
                c.x = x_tensor.data_ptr() + (d.x - x_base)
                if x_stride is not None:
                    c.x_stride = x_stride
                ent._descs.append(c)
            ent._rows = self._rows
            ent._keep = list(self._keep)
            ent._upload()
            cache[key] = ent
        ent._keep_x = x_tensor
        return ent

    def run(self, B):
        if not self._descs:
            return
        if self._dev is None:
            self._upload()
        STYLE_EPOCHS[self.lane] += 1
        check(_lib.load().cips3d_linear_table(self._dev.data_ptr(), len(self._descs), self._rows, B, stream_ptr()),
              "cips3d_linear_table")

    def backward(self, B, out_base, dy_base, x_base, dx_base=None, need_dW=True, need_db=True):
        """Gradients of every head (cips3d_linear_table_bwd).  dy_base / dx_base mirror the forward's out / x buffers
        (dx_base is accumulated into: zero it first).  Returns (dW_flat, w_offsets (python list), db_flat).
        The kernels read x and write dW in 16-byte pieces and find a row's head with one ballot: a table they cannot take
        (a head whose in_dim or x_stride is no multiple of 4 or whose x is not 16-byte aligned, more than 64 heads) is
        refused here, before any launch."""
        if len(self._descs) > 64:
            raise RuntimeError(f"LinearTable.backward: {len(self._descs)} heads, the table backward takes at most 64")
        for i, d in enumerate(self._descs):
            if d.in_dim % 4 != 0 or d.x_stride % 4 != 0 or (d.x or 0) % 16 != 0:
                raise RuntimeError(f"LinearTable.backward: head {i} (in_dim {d.in_dim}, x_stride {d.x_stride}, x at byte "
                                   f"{(d.x or 0) % 16} of a 16-byte line): in_dim and x_stride must be multiples of 4 and x 16-byte aligned")
        if self._dev is None:
            self._upload()
        # the widest head sizes the columns kernel's grid (cips3d_linear_table_bwd's in_dim); every head loops over its own
        in_dim = max(d.in_dim for d in self._descs)
        offs, off = [], 0
        for d in self._descs:
            offs.append(off)
            off += d.out_dim * d.in_dim
        if getattr(self, "_woff_dev", None) is None or self._woff_dev.numel() != len(offs):
            self._woff_dev = torch.tensor(offs, dtype=torch.int64).to(self.device)
        dW = torch.empty(off, device=self.device) if need_dW else None
        db = torch.empty(self._rows, device=self.device) if need_db else None
        check(_lib.load().cips3d_linear_table_bwd(self._dev.data_ptr(), len(self._descs), self._rows, in_dim, B,
                                                  dev_ptr(out_base, "out"), dev_ptr(dy_base, "dy"), dev_ptr(x_base, "x"),
                                                  dev_ptr(dx_base, "dx", True), self._woff_dev.data_ptr(), dev_ptr(dW, "dW", True),
                                                  dev_ptr(db, "db", True), stream_ptr()), "cips3d_linear_table_bwd")
        return dW, offs, db


def camera_params(locations, img_size, fov_ang=6.0, dist_radius=0.12, up=None):
    """locations [B,2] -> extrinsics [B,3,4], focal/near/far [B,1,1] (reference return shapes)."""
    lib = _lib.load()
    B = locations.shape[0]
    dev = locations.device
    loc = locations.detach().float().contiguous()
    fov_t = None
    fov_s = 0.0
    if torch.is_tensor(fov_ang):
        fov_t = fov_ang.detach().float().reshape(-1).contiguous()
        if fov_t.numel() == 1 and B != 1:
            fov_t = fov_t.expand(B).contiguous()
    else:
        fov_s = float(fov_ang)
    up_t = up.detach().float().contiguous() if up is not None else None
    extr = torch.empty(B, 3, 4, device=dev)
    focal = torch.empty(B, 1, 1, device=dev)
    near = torch.empty(B, 1, 1, device=dev)
    far = torch.empty(B, 1, 1, device=dev)
    check(lib.cips3d_camera_params(dev_ptr(loc, "locations"), dev_ptr(fov_t, "fov", True), fov_s, dev_ptr(up_t, "up", True),
                                   float(dist_radius), int(img_size), B, dev_ptr(extr), dev_ptr(focal), dev_ptr(near),
                                   dev_ptr(far), stream_ptr()), "cips3d_camera_params")
    return extr, focal, near, far


def _fov_arg(fov_ang, B):
    """fov_ang as the camera entry points take it: (a [B] float32 tensor | None, the scalar used when it is None)."""
    if not torch.is_tensor(fov_ang):
        return None, float(fov_ang)
    fov_t = fov_ang.detach().float().reshape(-1).contiguous()
    if fov_t.numel() == 1 and B != 1:
        fov_t = fov_t.expand(B).contiguous()
    if fov_t.numel() != B:
        raise ValueError(f"fov_ang tensor must have 1 or {B} elements, got {fov_t.numel()}")
    return fov_t, 0.0


def camera_axis_angle(rot, trans, img_size, fov_ang=6.0, dist_radius=0.12):
    """The free camera (cips3d_camera_axis_angle, csrc/camera_free.hip): rot [B,3] axis-angle, trans [B,3] -> extrinsics
    [B,3,4] = [exp([rot]x) | normalize(trans)], focal/near/far [B,1,1] (the shapes of camera_params).  One launch."""
    lib = _lib.load()
    B, dev = rot.shape[0], rot.device
    if tuple(rot.shape) != (B, 3) or tuple(trans.shape) != (B, 3):
        raise ValueError(f"camera_axis_angle: rot and trans must be [B,3], got {list(rot.shape)} and {list(trans.shape)}")
    r, t = rot.detach().float().contiguous(), trans.detach().float().contiguous()
    fov_t, fov_s = _fov_arg(fov_ang, B)
    extr = torch.empty(B, 3, 4, device=dev)
    focal, near, far = (torch.empty(B, 1, 1, device=dev) for _ in range(3))
    check(lib.cips3d_camera_axis_angle(dev_ptr(r, "rot"), dev_ptr(t, "trans"), dev_ptr(fov_t, "fov", True), fov_s,
                                       float(dist_radius), int(img_size), B, dev_ptr(extr), dev_ptr(focal), dev_ptr(near),
                                       dev_ptr(far), stream_ptr()), "cips3d_camera_axis_angle")
    return extr, focal, near, far


def camera_axis_angle_bwd(rot, trans, img_size, fov_ang, dextr=None, dfocal=None, need_dfov=None):
    """Backward of camera_axis_angle: dextr [B,3,4] and dfocal [B] (each may be None = zero) -> (drot [B,3], dtrans [B,3],
    dfov [B] | None).  need_dfov: None = when dfocal is given."""
    lib = _lib.load()
    B, dev = rot.shape[0], rot.device
    r, t = rot.detach().float().contiguous(), trans.detach().float().contiguous()
    fov_t, fov_s = _fov_arg(fov_ang, B)
    de = None if dextr is None else dextr.float().reshape(B, 3, 4).contiguous()
    df = None if dfocal is None else dfocal.float().reshape(B).contiguous()
    drot, dtrans = torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
    dfov = torch.empty(B, device=dev) if (df is not None if need_dfov is None else need_dfov) else None
    check(lib.cips3d_camera_axis_angle_bwd(dev_ptr(r, "rot"), dev_ptr(t, "trans"), dev_ptr(fov_t, "fov", True), fov_s,
                                           int(img_size), dev_ptr(de, "dextr", True), dev_ptr(df, "dfocal", True), B,
                                           dev_ptr(drot), dev_ptr(dtrans), dev_ptr(dfov, "dfov", True), stream_ptr()),
          "cips3d_camera_axis_angle_bwd")
    return drot, dtrans, dfov


def nerf_pack_weights(w_hidden, w_view, hidden, depth):
    lib = _lib.load()
    packed = torch.empty(int(lib.cips3d_nerf_packed_floats(hidden, depth)), device=w_view.device, dtype=torch.float32)
    check(lib.cips3d_nerf_pack_weights(dev_ptr(w_hidden, "w_hidden", True), dev_ptr(w_view, "w_view"), dev_ptr(packed),
                                       hidden, depth, stream_ptr()), "cips3d_nerf_pack_weights")
    return packed


def nerf_pack_weights32(w_hidden, w_view, hidden, depth):
    """The exact-fp32 weight stream (cips3d_nerf_params.packed32): fp32 A fragments of v_mfma_f32_16x16x4_f32."""
    lib = _lib.load()
    packed = torch.empty(int(lib.cips3d_nerf_packed_floats(hidden, depth)), device=w_view.device, dtype=torch.float32)
    check(lib.cips3d_nerf_pack_weights32(dev_ptr(w_hidden, "w_hidden", True), dev_ptr(w_view, "w_view"), dev_ptr(packed),
                                         hidden, depth, stream_ptr()), "cips3d_nerf_pack_weights32")
    return packed


def nerf_suggest_chunks(B, img_size, n_samples):
    return int(_lib.load().cips3d_nerf_suggest_chunks(B, img_size, n_samples))


def _nerf_params(kw):
    p = _lib.NerfParams()
    ptr_fields = ("near_", "far_", "w_first", "packed", "w_view", "film", "layer_bias",
                  "w_sigma", "w_rgb", "b_sigma", "b_rgb", "sigmoid_beta")
    for f in ptr_fields:
        setattr(p, f, dev_ptr(kw[f], f))
    p.packed32 = dev_ptr(kw.get("packed32"), "packed32", True)          # exact-fp32 arithmetic (csrc/nerf.hip, F32 instantiation)
    p.part = dev_ptr(kw.get("part"), "part", True)
    for f in ("cam_poses", "focals"):
        setattr(p, f, dev_ptr(kw.get(f), f, kw.get("x_pts") is not None))
    p.perturb_u = dev_ptr(kw.get("perturb_u"), "perturb_u", True)
    p.sdf = dev_ptr(kw.get("sdf"), "sdf", True)
    for f in ("stash", "bwd_sdf", "bwd_crgb"):                        # differentiable forward (cips3d_nerf_bwd_fused's inputs)
        setattr(p, f, dev_ptr(kw.get(f), f, True))
    for f in ("x_pts", "x_rays_d", "x_viewdirs", "x_z_vals"):          # explicit-geometry mode
        setattr(p, f, dev_ptr(kw.get(f), f, True))
    p.n_rays = int(kw.get("n_rays", 0))
    zw = kw.get("zero_words")                                          # float scratch the launch leaves zeroed (cips3d_nerf_params.zero_words)
    if zw is not None:
        p.zero_words, p.n_zero_words = dev_ptr(zw, "zero_words"), zw.numel()
    p.raw_density = int(bool(kw.get("raw_density", False)))            # with_sdf = False (backward: sigmoid_beta = None)
    for f in ("B", "img_size", "n_samples", "hidden", "depth", "static_viewdirs", "n_chunks"):
        setattr(p, f, int(kw[f]))
    return p


def nerf_render(**kw):
    """Fill cips3d_nerf_params from keyword tensors / ints and launch the fused renderer (chunk partials -> `part`)."""
    lib = _lib.load()
    if kw.get("part") is None:
        raise RuntimeError("part is required")
    p = _nerf_params(kw)
    ev = _timed("nerf_render")
    check(lib.cips3d_nerf_render(C.byref(p), stream_ptr()), "cips3d_nerf_render")
    if ev:
        ev[1].record()


def nerf_render_maps(**kw):
    """Renderer + ordered combination of the chunk partials -> (features, thumb, xyz, mask), [B,C,S,S] (or [B,C,n_rays,1] in
    explicit-geometry mode).  The render kernel combines the partials itself when cips3d_nerf_fuses_finish says so; else
    they go through `part` and cips3d_nerf_finish."""
    lib = _lib.load()
    p = _nerf_params(kw)
    B, H, S, n_rays = p.B, p.hidden, p.img_size, p.n_rays
    dev = kw["near_"].device
    shp = (n_rays, 1) if n_rays > 0 else (S, S)
    features = torch.empty(B, H, *shp, device=dev)
    thumb, xyz = torch.empty(B, 3, *shp, device=dev), torch.empty(B, 3, *shp, device=dev)
    mask = torch.empty(B, 2, *shp, device=dev)
    p.o_features, p.o_thumb, p.o_xyz, p.o_mask = dev_ptr(features), dev_ptr(thumb), dev_ptr(xyz), dev_ptr(mask)
    fused = bool(lib.cips3d_nerf_fuses_finish(C.byref(p)))
    planar = bool(kw.get("planar_mask"))          # mask as [2,B,...]: written that way by the fused finish, one transposing copy otherwise
    if planar and fused:
        mask = torch.empty(2, B, *shp, device=dev)
        p.o_mask, p.mask_planar = dev_ptr(mask), 1
    part = None
    if not fused:
        R = n_rays if n_rays > 0 else S * S
        part = torch.empty(p.n_chunks, B, H + 8, R, device=dev)
        p.part = dev_ptr(part)
    ev = _timed("nerf_render")
    check(lib.cips3d_nerf_render(C.byref(p), stream_ptr()), "cips3d_nerf_render")
    if ev:
        ev[1].record()
    if not fused:
        check(lib.cips3d_nerf_finish_rays(p.part, p.n_chunks, B, n_rays if n_rays > 0 else S * S, H, dev_ptr(features),
                                          dev_ptr(thumb), dev_ptr(xyz), dev_ptr(mask), stream_ptr()), "cips3d_nerf_finish_rays")
        if planar:
            mask = mask.transpose(0, 1).contiguous()
    return features, thumb, xyz, mask


def nerf_sdf_grad_supported(hidden, depth):
    """Host-only: does cips3d_nerf_sdf_grad implement this trunk (hidden 256, depth 1..64)?"""
    return bool(_lib.load().cips3d_nerf_sdf_grad_supported(int(hidden), int(depth)))


def nerf_sdf_grad(*, near_, far_, w_first, packed32, film, layer_bias, w_sigma, b_sigma, B, n_samples, hidden, depth,
                  img_size=1, cam_poses=None, focals=None, perturb_u=None, x_pts=None, n_rays=0, want_sdf=True, grad_out=None,
                  sdf_out=None):
    """d sdf / d pts at every sample point (csrc/nerf_sdf_grad.hip) -> (sdf [B,R,N] or None, grad [B,R,N,3]).  Camera form
    (cam_poses, focals, img_size[, perturb_u]: the sample positions of nerf_render for the same arguments) or explicit form
    (x_pts [B,R,N,3], n_rays = R).  grad_out / sdf_out: contiguous fp32 tensors of those shapes to write into."""
    lib = _lib.load()
    if not lib.cips3d_nerf_sdf_grad_supported(int(hidden), int(depth)):
        raise NotImplementedError(f"the SDF gradient kernel is built for hidden_dim = 256 and depth <= 64 (got hidden {hidden}, "
                                  f"depth {depth})")
    p = _lib.NerfParams()
    for f, t in (("near_", near_), ("far_", far_), ("w_first", w_first), ("film", film), ("layer_bias", layer_bias),
                 ("w_sigma", w_sigma), ("b_sigma", b_sigma)):
        setattr(p, f, dev_ptr(t, f))
    p.packed32 = dev_ptr(packed32, "packed32", depth == 1)
    explicit = x_pts is not None
    p.cam_poses, p.focals = dev_ptr(cam_poses, "cam_poses", explicit), dev_ptr(focals, "focals", explicit)
    p.perturb_u = dev_ptr(perturb_u, "perturb_u", True)
    p.x_pts = dev_ptr(x_pts, "x_pts", True)
    p.n_rays = int(n_rays) if explicit else 0
    p.B, p.img_size, p.n_samples, p.hidden, p.depth, p.n_chunks = int(B), int(img_size), int(n_samples), int(hidden), int(depth), 1
    R = p.n_rays if explicit else p.img_size * p.img_size
    dev = near_.device
    grad = torch.empty(p.B, R, p.n_samples, 3, device=dev) if grad_out is None else grad_out
    sdf = sdf_out if sdf_out is not None else (torch.empty(p.B, R, p.n_samples, device=dev) if want_sdf else None)
    if tuple(grad.shape) != (p.B, R, p.n_samples, 3) or (sdf is not None and tuple(sdf.shape) != (p.B, R, p.n_samples)):
        raise RuntimeError(f"grad_out / sdf_out must have shapes {(p.B, R, p.n_samples, 3)} / {(p.B, R, p.n_samples)}")
    p.sdf = dev_ptr(sdf, "sdf", True)
    ev = _timed("nerf_sdf_grad")
    check(lib.cips3d_nerf_sdf_grad(C.byref(p), dev_ptr(grad), stream_ptr()), "cips3d_nerf_sdf_grad")
    if ev:
        ev[1].record()
    return sdf, grad


def nerf_eikonal_supported(hidden, depth):
    """Host-only: does cips3d_nerf_eikonal_loss implement this trunk (hidden 256, depth 1..64)?"""
    return bool(_lib.load().cips3d_nerf_eikonal_supported(int(hidden), int(depth)))


def nerf_eikonal_workspace_bytes(hidden, depth, workgroups, values_only=False):
    """Host-only: bytes of cips3d_nerf_eikonal_loss's workspace for a grid of at most `workgroups` workgroups."""
    return int(_lib.load().cips3d_nerf_eikonal_workspace_bytes(int(hidden), int(depth), int(workgroups), int(bool(values_only))))


def nerf_eikonal_workspace(hidden, depth, B, device, values_only=False):
    """The workspace nerf_eikonal_loss allocates when none is passed: room for compute units + B workgroups, 192 KB x depth each
    (about 50 MB x depth on 256 compute units).  It comes from torch's caching allocator, so a loop that calls every step reuses
    one block; a caller that wants to hold it passes it in."""
    wgs = torch.cuda.get_device_properties(device).multi_processor_count + int(B)
    return torch.empty(nerf_eikonal_workspace_bytes(hidden, depth, wgs, values_only), device=device, dtype=torch.uint8)


def nerf_eikonal_loss(*, near_, far_, w_first, packed32, packed32_t, film, layer_bias, w_sigma, b_sigma, B, n_samples, hidden, depth,
                      img_size=1, cam_poses=None, focals=None, perturb_u=None, x_pts=None, n_rays=0, lambda_eikonal=1.0,
                      lambda_minimal_surface=1.0, beta=100.0, values_only=False, dfilm_out=None, workspace=None):
    """The eikonal loss mean((|d sdf / d pts| - 1)^2) and the minimal-surface loss mean(exp(-beta |sdf|)) over the B R N sample
    points of a call, with d (lambda_eikonal eik + lambda_minimal_surface ms) / d film (csrc/nerf_eikonal.hip)
    -> (loss [2] float64: the two UNWEIGHTED means, dfilm [B, depth+1, 2, hidden] or None with values_only).
    Geometry as nerf_sdf_grad: camera form or explicit form (x_pts [B,R,N,3], n_rays = R).  packed32_t: nerf_pack_weights32 of
    the transposed hidden matrices in reverse layer order (VolumeFeatureRenderer.packed32_t).  workspace: a uint8 tensor of
    nerf_eikonal_workspace_bytes(...) bytes, else nerf_eikonal_workspace(...) allocates one; its size decides the grid,
    and values and dfilm are bit-identical from run to run for one size."""
    lib = _lib.load()
    if not lib.cips3d_nerf_eikonal_supported(int(hidden), int(depth)):
        raise NotImplementedError(f"the eikonal loss kernel is built for hidden_dim = 256 and depth <= 64 (got hidden {hidden}, "
                                  f"depth {depth})")
    p = _lib.NerfParams()
    for f, t in (("near_", near_), ("far_", far_), ("w_first", w_first), ("film", film), ("layer_bias", layer_bias),
                 ("w_sigma", w_sigma), ("b_sigma", b_sigma)):
        setattr(p, f, dev_ptr(t, f))
    p.packed32 = dev_ptr(packed32, "packed32", depth == 1)
    explicit = x_pts is not None
    p.cam_poses, p.focals = dev_ptr(cam_poses, "cam_poses", explicit), dev_ptr(focals, "focals", explicit)
    p.perturb_u = dev_ptr(perturb_u, "perturb_u", True)
    p.x_pts = dev_ptr(x_pts, "x_pts", True)
    p.n_rays = int(n_rays) if explicit else 0
    p.B, p.img_size, p.n_samples, p.hidden, p.depth, p.n_chunks = int(B), int(img_size), int(n_samples), int(hidden), int(depth), 1
    dev = near_.device
    if tuple(film.shape) != (p.B, p.depth + 1, 2, p.hidden):
        raise RuntimeError(f"film must have shape {(p.B, p.depth + 1, 2, p.hidden)}, got {tuple(film.shape)}")
    values_only = bool(values_only)
    if workspace is None:
        workspace = nerf_eikonal_workspace(hidden, depth, p.B, dev, values_only)
    loss = torch.empty(2, device=dev, dtype=torch.float64)
    dfilm = None
    if not values_only:
        dfilm = torch.empty(p.B, p.depth + 1, 2, p.hidden, device=dev) if dfilm_out is None else dfilm_out
        if tuple(dfilm.shape) != (p.B, p.depth + 1, 2, p.hidden):
            raise RuntimeError(f"dfilm_out must have shape {(p.B, p.depth + 1, 2, p.hidden)}")
    ev = _timed("nerf_eikonal_loss")
    check(lib.cips3d_nerf_eikonal_loss(C.byref(p), dev_ptr(packed32_t, "packed32_t", depth == 1 or values_only),
                                       float(lambda_eikonal), float(lambda_minimal_surface), float(beta), int(values_only),
                                       dev_ptr(workspace, "workspace", dtype=torch.uint8), workspace.numel(),
                                       dev_ptr(loss, "loss", dtype=torch.float64), dev_ptr(dfilm, "dfilm", values_only),
                                       stream_ptr()), "cips3d_nerf_eikonal_loss")
    if ev:
        ev[1].record()
    return loss, dfilm


PHONG_DEFAULTS = dict(ka=0.1, kd=0.65, ks=0.2, shininess=64.0)     # the reference's create_mesh_renderer; pytorch3d's shininess


def nerf_normals(*, sdf, grad, sigmoid_beta, B, n_samples, img_size=1, cam_poses=None, focals=None, near_=None, far_=None,
                 perturb_u=None, x_z_vals=None, x_rays_d=None, n_rays=0, xyz=None, eye=None, light=None, ka=None, kd=None,
                 ks=None, shininess=None, want=("normal_raw", "normal"), normal_raw_out=None, normal_out=None, shade_out=None,
                 shade_u8_out=None):
    """Composited normals / Phong-shaded frame (csrc/nerf_normals.hip) -> dict with the entries named in `want` (and every
    entry a `*_out` tensor was given for): normal_raw, normal [B,3,R] fp32, shade [B,R] fp32, shade_u8 [B,3,R] uint8.
    sdf [B,R,N], grad [B,R,N,3]: nerf_sdf_grad's outputs.  Camera form (cam_poses, focals, near_, far_, img_size[, perturb_u]) or
    explicit form (x_z_vals [B,R,N], x_rays_d [B,R,3], n_rays = R).  The shade outputs need xyz [B,3,R], eye [B,3], light [B,3];
    ka / kd / ks / shininess default to PHONG_DEFAULTS."""
    lib = _lib.load()
    outs = {"normal_raw": normal_raw_out, "normal": normal_out, "shade": shade_out, "shade_u8": shade_u8_out}
    names = [n for n in outs if n in want or outs[n] is not None]
    unknown = [n for n in want if n not in outs]
    if unknown or not names:
        raise RuntimeError(f"nerf_normals: want must name some of {tuple(outs)}, got {tuple(want)}")
    if any(n in names for n in ("shade", "shade_u8")) and (xyz is None or eye is None or light is None):
        raise RuntimeError("nerf_normals: the shade outputs need xyz, eye and light")
    explicit = x_z_vals is not None
    p = _lib.NormalsParams()
    p.sdf, p.grad, p.sigmoid_beta = dev_ptr(sdf, "sdf"), dev_ptr(grad, "grad"), dev_ptr(sigmoid_beta, "sigmoid_beta")
    for f, t in (("cam_poses", cam_poses), ("focals", focals), ("near_", near_), ("far_", far_)):
        setattr(p, f, dev_ptr(t, f, explicit))
    p.perturb_u = dev_ptr(perturb_u, "perturb_u", True)
    p.x_z_vals, p.x_rays_d = dev_ptr(x_z_vals, "x_z_vals", True), dev_ptr(x_rays_d, "x_rays_d", not explicit)
    p.xyz, p.eye, p.light = dev_ptr(xyz, "xyz", True), dev_ptr(eye, "eye", True), dev_ptr(light, "light", True)
    p.B, p.img_size, p.n_samples, p.n_rays = int(B), int(img_size), int(n_samples), int(n_rays) if explicit else 0
    R = p.n_rays if explicit else p.img_size * p.img_size
    if tuple(sdf.shape) != (p.B, R, p.n_samples) or tuple(grad.shape) != (p.B, R, p.n_samples, 3):
        raise RuntimeError(f"nerf_normals: sdf / grad must have shapes {(p.B, R, p.n_samples)} / {(p.B, R, p.n_samples, 3)}")
    for name, t, shape in (("perturb_u", perturb_u, (p.B, R)), ("x_z_vals", x_z_vals, (p.B, R, p.n_samples)),
                           ("x_rays_d", x_rays_d, (p.B, R, 3)), ("xyz", xyz, (p.B, 3, R)), ("eye", eye, (p.B, 3)),
                           ("light", light, (p.B, 3))):
        if t is not None and t.numel() != _numel(shape):
            raise RuntimeError(f"nerf_normals: {name} must have {_numel(shape)} elements {shape}, got {tuple(t.shape)}")
    dev = sdf.device
    shapes = {"normal_raw": (p.B, 3, R), "normal": (p.B, 3, R), "shade": (p.B, R), "shade_u8": (p.B, 3, R)}
    ret = {}
    for n in names:
        dt = torch.uint8 if n == "shade_u8" else torch.float32
        t = outs[n] if outs[n] is not None else torch.empty(shapes[n], device=dev, dtype=dt)
        if t.numel() != _numel(shapes[n]):
            raise RuntimeError(f"nerf_normals: {n}_out must have {_numel(shapes[n])} elements {shapes[n]}, got {tuple(t.shape)}")
        setattr(p, n, dev_ptr(t, n + "_out", dtype=dt))
        ret[n] = t
    ph = dict(PHONG_DEFAULTS)
    ph.update({k: v for k, v in (("ka", ka), ("kd", kd), ("ks", ks), ("shininess", shininess)) if v is not None})
    p.ka, p.kd, p.ks, p.shininess = (float(ph[k]) for k in ("ka", "kd", "ks", "shininess"))
    ev = _timed("nerf_normals")
    check(lib.cips3d_nerf_normals(C.byref(p), stream_ptr()), "cips3d_nerf_normals")
    if ev:
        ev[1].record()
    return ret


def _numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def rays_in_world(cam_poses, focals, img_size, static_viewdirs=False):
    """-> rays_o, rays_d, viewdirs, each [B,S,S,3] (Render.get_rays_in_world)."""
    lib = _lib.load()
    B = cam_poses.shape[0]
    o, d, v = (torch.empty(B, img_size, img_size, 3, device=cam_poses.device) for _ in range(3))
    c2w, foc = cam_poses.float().contiguous(), focals.float().reshape(B).contiguous()     # converted copies live until the launch
    check(lib.cips3d_rays_in_world(dev_ptr(c2w, "c2w"), dev_ptr(foc, "focal"),
                                   img_size, int(bool(static_viewdirs)), B, dev_ptr(o), dev_ptr(d), dev_ptr(v), stream_ptr()),
          "cips3d_rays_in_world")
    return o, d, v


def z_vals(near, far, B, R, N, perturb_u=None, stratified=False):
    """offset sampling (perturb_u: one uniform per ray, [B,R]) or, stratified=True, the classic stratified branch (perturb_u:
    one uniform per sample, [B,R,N])."""
    lib = _lib.load()
    z = torch.empty(B, R, N, device=near.device)
    nr, fr = near.float().reshape(B).contiguous(), far.float().reshape(B).contiguous()   # converted copies live until the launch
    if stratified:
        u = None if perturb_u is None else perturb_u.float().reshape(B, R, N).contiguous()
        check(lib.cips3d_z_vals_stratified(dev_ptr(nr, "near"), dev_ptr(fr, "far"), dev_ptr(u, "u", True), B, R, N, dev_ptr(z),
                                           stream_ptr()), "cips3d_z_vals_stratified")
        return z
    u = None if perturb_u is None else perturb_u.float().reshape(B, R).contiguous()
    check(lib.cips3d_z_vals(dev_ptr(nr, "near"), dev_ptr(fr, "far"),
                            dev_ptr(u, "u", True), B, R, N, dev_ptr(z), stream_ptr()), "cips3d_z_vals")
    return z


def ray_points(rays_o, rays_d, z, near=None, far=None, want_pts=True, want_normalized=False):
    """rays [B,R,3], z [B,R,N] -> pts and/or normalised pts [B,R,N,3]."""
    lib = _lib.load()
    B, R, N = z.shape
    dev = z.device
    pts = torch.empty(B, R, N, 3, device=dev) if want_pts else None
    ptsn = torch.empty(B, R, N, 3, device=dev) if want_normalized else None
    nr = None if near is None else near.float().reshape(B).contiguous()
    fr = None if far is None else far.float().reshape(B).contiguous()
    check(lib.cips3d_ray_points(dev_ptr(rays_o, "rays_o"), dev_ptr(rays_d, "rays_d"), dev_ptr(z, "z_vals"), dev_ptr(nr, "near", True),
                                dev_ptr(fr, "far", True), B, R, N, dev_ptr(pts, "pts", True), dev_ptr(ptsn, "ptsn", True),
                                stream_ptr()), "cips3d_ray_points")
    return pts, ptsn


VI_RAW_DENSITY, VI_FORCE_BACKGROUND = 1, 2


def volume_integration(rgb, sdf, features, z, rays_d, pts, sigmoid_beta, raw_density=False, force_background=False):
    """[n,N,3], [n,N], [n,N,C]|None, [n,N], [n,3], [n,N,3] -> rgb_map [n,3], feature_map [n,C]|None, xyz [n,3], mask [n,2].
    raw_density: `sdf` is the raw density output (softplus branch, with_sdf=False); force_background: nerf_utils.py:309-310."""
    lib = _lib.load()
    n, N = z.shape
    dev = z.device
    Cc = features.shape[-1] if features is not None else 0
    rgb_map, xyz, mask = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 2, device=dev)
    fmap = torch.empty(n, Cc, device=dev) if features is not None else None
    check(lib.cips3d_volume_integration(dev_ptr(rgb, "rgb"), dev_ptr(sdf, "sdf"), dev_ptr(features, "features", True),
                                        dev_ptr(z, "z_vals"), dev_ptr(rays_d, "rays_d"), dev_ptr(pts, "pts"),
                                        dev_ptr(sigmoid_beta, "sigmoid_beta", raw_density), n, N, Cc,
                                        (VI_RAW_DENSITY if raw_density else 0) | (VI_FORCE_BACKGROUND if force_background else 0),
                                        dev_ptr(rgb_map),
                                        dev_ptr(fmap, "feature_map", True), dev_ptr(xyz), dev_ptr(mask), stream_ptr()),
          "cips3d_volume_integration")
    return rgb_map, fmap, xyz, mask


def points_linear(x, W, bias=None, film=None, out_scale=1.0, out_shift=0.0):
    """x (b, ..., in) point-major -> (b, ..., out): LinearLayer (film None) or FiLMSiren (film [B,2,out] = gamma, beta)."""
    lib = _lib.load()
    xin = x.float().contiguous()
    B, in_dim = xin.shape[0], xin.shape[-1]
    n = xin.numel() // in_dim
    out_dim = W.shape[0]
    y = torch.empty(*xin.shape[:-1], out_dim, device=x.device)
    check(lib.cips3d_points_linear(dev_ptr(xin, "x"), dev_ptr(W, "W"), dev_ptr(bias, "bias", True), dev_ptr(film, "film", True), n,
                                   max(1, n // B), in_dim, out_dim, 0 if film is None else 1, float(out_scale), float(out_shift),
                                   dev_ptr(y), stream_ptr()), "cips3d_points_linear")
    return y


def nerf_finish(part, n_chunks, B, img_size, hidden, n_rays=None):
    lib = _lib.load()
    dev = part.device
    if n_rays is not None:           # explicit-geometry mode: a [B, C, n_rays, 1] "image"
        features = torch.empty(B, hidden, n_rays, 1, device=dev)
        thumb, xyz = torch.empty(B, 3, n_rays, 1, device=dev), torch.empty(B, 3, n_rays, 1, device=dev)
        mask = torch.empty(B, 2, n_rays, 1, device=dev)
        check(lib.cips3d_nerf_finish_rays(dev_ptr(part), n_chunks, B, n_rays, hidden, dev_ptr(features), dev_ptr(thumb),
                                          dev_ptr(xyz), dev_ptr(mask), stream_ptr()), "cips3d_nerf_finish_rays")
        return features, thumb, xyz, mask
    R = img_size * img_size
    features = torch.empty(B, hidden, img_size, img_size, device=dev)
    thumb = torch.empty(B, 3, img_size, img_size, device=dev)
    xyz = torch.empty(B, 3, img_size, img_size, device=dev)
    mask = torch.empty(B, 2, img_size, img_size, device=dev)
    check(lib.cips3d_nerf_finish(dev_ptr(part), n_chunks, B, img_size, hidden, dev_ptr(features), dev_ptr(thumb),
                                 dev_ptr(xyz), dev_ptr(mask), stream_ptr()), "cips3d_nerf_finish")
    return features, thumb, xyz, mask


def modulate_weights(W, s, s_stride, B, Cout, Cin, ksq, scale, demodulate, packed, s_offset=0, out=None, flip=False,
                     split=False, bf16=False):
    lib = _lib.load()
    if out is None:
        # (the 3x3 kernel's split-fp16 tap-pair fragments hold ten taps per weight row: five pairs, the tenth tap zero)
        out = torch.empty(B * Cout * Cin * (10 if (split and packed and ksq == 9) else ksq), device=W.device, dtype=torch.float32)
    flags = ((MOD_DEMODULATE if demodulate else 0) | (MOD_PACKED if packed else 0) | (MOD_FLIP if flip else 0) |
             (MOD_SPLIT if split else 0) | (MOD_BF16 if bf16 else 0))
    check(lib.cips3d_modulate_weights(dev_ptr(W, "W"), dev_ptr(s, "s") + 4 * s_offset, s_stride, dev_ptr(out), B, Cout, Cin,
                                      ksq, float(scale), flags, stream_ptr()), "cips3d_modulate_weights")
    return out


def modconv1x1_supported(Cin, Cout, HW):
    return bool(_lib.load().cips3d_modconv1x1_supported(Cin, Cout, HW))


# ---- range tracking of the split-fp16 modes (cips3d_range, include/cips3d_hip.h): every split happens on x * 2^-e with a power
# of two per (tensor, sample) taken from a bound of max|x|, so that the decoder's default arithmetic keeps fp32's exponent
# range.  amax arrays are [B, AMAX_FLOATS] fp32 tensors; a kernel that produced a tensor leaves its amax attached to it
# (`tag_amax`), a split GEMM that reads an untagged tensor measures it first (one HBM pass).
def amax_floats():
    """floats per sample of an amax array (CIPS3D_AMAX_SLOTS * CIPS3D_AMAX_STRIDE of the loaded library)"""
    _lib.load()
    return _lib.AMAX_FLOATS


NOISE_BOUND_RNG = 6.0        # cips3d_rng_fill: |n| <= sqrt(50 ln 2) = 5.89
NOISE_BOUND_TORCH = 7.0      # torch.randn on the device: Box-Muller on 32-bit uniforms, |n| <= 6.8


def new_amax(B, device):
    return torch.zeros(B, amax_floats(), device=device, dtype=torch.float32)


def absmax(x, B=None):
    """amax array of x viewed as [B, -1] (B defaults to x.shape[0])."""
    B = x.shape[0] if B is None else B
    x = x.contiguous()
    amax = torch.empty(B, amax_floats(), device=x.device, dtype=torch.float32)
    check(_lib.load().cips3d_absmax(dev_ptr(x, "x"), B, x.numel() // B, dev_ptr(amax), stream_ptr()), "cips3d_absmax")
    return amax


def amax_value(amax):
    """[B] tensor of the maxima an amax array holds (tests, diagnostics)."""
    return amax.view(amax.shape[0], _lib.AMAX_SLOTS, _lib.AMAX_STRIDE)[:, :, 0].max(dim=1).values


def tag_amax(t, amax):
    """Remember the amax array of tensor t (valid while t is not modified in place)."""
    t._cips3d_amax = (amax, t._version)
    return t


def amax_of(t, measure=True):
    tag = getattr(t, "_cips3d_amax", None)
    if tag is not None and tag[1] == t._version and tag[0].shape[0] == t.shape[0]:
        return tag[0]
    return absmax(t) if measure else None


_const_amax = {}


def const_amax(B, bound, device):
    """amax array of a tensor whose bound is known a priori (sines: 1)."""
    key = (B, float(bound), str(device))
    t = _const_amax.get(key)
    if t is None:
        t = _const_amax[key] = torch.full((B, amax_floats()), float(bound), device=device, dtype=torch.float32)
    return t


def range_consts(B, bias, noise_w, w_gain, fir=None, noise=None, noise_bound=0.0):
    """lconst [B, 4] of one StyledConv (cips3d_range_consts).  The bound of |noise| is measured from `noise` (a device tensor)
    when given -- no host round trip -- and / or taken from `noise_bound`."""
    lib = _lib.load()
    dev = bias.device
    lconst = torch.empty(B, 4, device=dev, dtype=torch.float32)
    na = absmax(noise, B=1) if noise is not None else None
    bflat = bias.contiguous().view(-1)
    check(lib.cips3d_range_consts(dev_ptr(bflat, "bias"), bflat.numel(), dev_ptr(noise_w, "noise_w", True), float(noise_bound),
                                  dev_ptr(na, "noise_amax", True), float(w_gain), dev_ptr(fir, "fir", True), dev_ptr(lconst), B,
                                  stream_ptr()), "cips3d_range_consts")
    return lconst


def _range(**kw):
    rg = _lib.Range()
    keep = []
    for k, v in kw.items():
        if v is not None:
            keep.append(v)
            setattr(rg, k, v.data_ptr())
    return rg, keep


GEMM_BF16 = 0x100      # CIPS3D_GEMM_BF16: bf16 compute mode of the decoder GEMMs (BASELINE config 3)
Y_BF16 = 0x200         # CIPS3D_Y_BF16: the pre-FIR low-resolution GEMM result of an up-sampling stage is stored as bf16
GEMM_SPLIT = 0x400     # CIPS3D_GEMM_SPLIT: fp32-equivalent split-fp16 products (weights packed with MOD_SPLIT)
RGB_U8 = 0x800         # CIPS3D_RGB_U8: the fused stage stores its image as uint8 (cips3d_rgb_to_uint8 of the value it would have stored)
STAGE_FLAT = 0x1000    # CIPS3D_STAGE_FLAT: the fused stage kernel on a block that does not up-sample


def modconv1x1(x, wm_packed, Cout, epilogue=0, noise=None, noise_w=None, bias=None, out=None, bf16=False, out_bf16=False,
               split=False, x_amax=None, track=None):
    """out_bf16 (epilogue 0 only): the result is stored as a torch.bfloat16 tensor (CIPS3D_Y_BF16).
    split: fp32-equivalent split-fp16 products; wm_packed must come from modulate_weights(..., packed=True, split=True).
    The activations are split as x * 2^-e (cips3d_range): x_amax = the amax array of x, else the one attached to x by the kernel
    that made it, else measured here.  track (default: split): leave the output's amax attached to the result."""
    lib = _lib.load()
    B, Cin, H, W = x.shape
    if split and x_amax is None:
        x_amax = amax_of(x)
    if track is None:
        track = split
    out_amax = new_amax(B, x.device) if (track and not out_bf16) else None
    rg, _keep = _range(x_amax=x_amax if split else None, out_amax=out_amax)
    odt = torch.bfloat16 if out_bf16 else torch.float32
    if out is None:
        out = torch.empty(B, Cout, H, W, device=x.device, dtype=odt)
    nb = 0
    if noise is not None and noise.shape[0] == B and B > 1:
        nb = H * W
    if noise is not None and noise.shape[0] not in (1, B):
        raise RuntimeError("noise batch must be 1 or B")
    check(lib.cips3d_modconv1x1(dev_ptr(x, "x"), dev_ptr(wm_packed, "wm"), dev_ptr(out, "out", dtype=odt), B, Cin, Cout, H * W,
                                epilogue | (GEMM_BF16 if bf16 else 0) | (Y_BF16 if out_bf16 else 0) | (GEMM_SPLIT if split else 0),
                                dev_ptr(noise, "noise", True), nb, dev_ptr(noise_w, "noise_w", True), dev_ptr(bias, "bias", True),
                                C.byref(rg), stream_ptr()), "cips3d_modconv1x1")
    if out_amax is not None:
        tag_amax(out, out_amax)
    return out


def up2_fir_act(y_lo, fir, noise, noise_w, bias, out=None, track=False):
    """track: the kernel records the output's amax array (cips3d_range) and leaves it attached to the result."""
    lib = _lib.load()
    B, Cc, H, W = y_lo.shape
    if out is None:
        out = torch.empty(B, Cc, 2 * H, 2 * W, device=y_lo.device, dtype=torch.float32)
    nb = 4 * H * W if (noise is not None and noise.shape[0] == B and B > 1) else 0
    out_amax = new_amax(B, y_lo.device) if track else None
    check(lib.cips3d_up2_fir_act(dev_ptr(y_lo, "y_lo"), dev_ptr(fir, "fir"), dev_ptr(out), B, Cc, H, W,
                                 dev_ptr(noise, "noise", True), nb, dev_ptr(noise_w, "noise_w", True), dev_ptr(bias, "bias"),
                                 dev_ptr(out_amax, "out_amax", True), stream_ptr()), "cips3d_up2_fir_act")
    if out_amax is not None:
        tag_amax(out, out_amax)
    return out


def noise_bias_act(x, noise, noise_w, bias):
    lib = _lib.load()
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    nb = H * W if (noise is not None and noise.shape[0] == B and B > 1) else 0
    check(lib.cips3d_noise_bias_act(dev_ptr(x, "x"), dev_ptr(noise, "noise", True), nb, dev_ptr(noise_w, "noise_w", True), dev_ptr(bias, "bias"),
                                    dev_ptr(out), B, Cc, H * W, stream_ptr()), "cips3d_noise_bias_act")
    return out


def torgb(x, wm, bias, skip=None, skip_up=False, fir=None, out=None):
    lib = _lib.load()
    B, Cin, H, W = x.shape
    if out is None:
        out = torch.empty(B, 3, H, W, device=x.device, dtype=torch.float32)
    check(lib.cips3d_torgb(dev_ptr(x, "x"), dev_ptr(wm, "wm"), dev_ptr(bias, "bias"), dev_ptr(skip, "skip", True),
                           int(bool(skip_up)), dev_ptr(fir, "fir", True), dev_ptr(out), B, Cin, H, W, stream_ptr()),
          "cips3d_torgb")
    return out


def modconv_kxk(x, wm, Cout, k, transpose2=False):
    lib = _lib.load()
    B, Cin, H, W = x.shape
    OH = 2 * H - 1 + k - 1 if transpose2 else H
    OW = 2 * W - 1 + k - 1 if transpose2 else W
    out = torch.empty(B, Cout, OH, OW, device=x.device, dtype=torch.float32)
    check(lib.cips3d_modconv_kxk(dev_ptr(x, "x"), dev_ptr(wm, "wm"), dev_ptr(out), B, Cin, Cout, H, W, k,
                                 int(bool(transpose2)), stream_ptr()), "cips3d_modconv_kxk")
    return out


def _given(t, shape, dtype, device, make):
    """the caller's output tensor `t` after a check of its shape and type, or a fresh make(shape)"""
    if t is None:
        return make(*shape, device=device, dtype=dtype)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device.type != torch.device(device).type:
        raise RuntimeError(f"an output tensor must be a contiguous {dtype} tensor of shape {tuple(shape)} on the device")
    return t


def planes_supported(Cin, Cout, HW):
    return bool(_lib.load().cips3d_planes_supported(Cin, Cout, HW))


def to_planes(x, ranged=True, out=None, out_exp=None, out_pmax=None):
    """fp32 [B,C,H,W] -> split-fp16 planes (torch.float16 tensor [B, C/8, 2, H*W, 8]: hi plane, lo plane) of x * 2^-e, e one
    power of two per sample that puts max|x| into [2^14, 2^15) (cips3d_range).  The exponents ([B, blocks of 128 pixels] int32:
    the format allows one per pixel block, this conversion writes the sample's everywhere) travel as an attribute of the
    result (`.cips3d_exp`); ranged=False stores x itself (e = 0).  out / out_exp / out_pmax: caller-supplied tensors of those
    shapes to write instead of fresh ones."""
    lib = _lib.load()
    B, Cc, H, W = x.shape
    p = _given(out, (B, Cc // 8, 2, H * W, 8), torch.float16, x.device, torch.empty)
    amax = amax_of(x) if ranged else None
    nblk = (H * W + _lib.PLANES_EXP_BLOCK - 1) // _lib.PLANES_EXP_BLOCK
    exps = _given(out_exp, (B, nblk), torch.int32, x.device, torch.zeros) if ranged else None
    pmax = _given(out_pmax, (B, (H * W + 63) // 64, Cc // 16), torch.float32, x.device, torch.zeros) \
        if (ranged and Cc % 16 == 0) else None
    check(lib.cips3d_to_planes(dev_ptr(x, "x"), p.data_ptr(), B, Cc, H * W, dev_ptr(amax, "amax", True),
                               exps.data_ptr() if ranged else None, dev_ptr(pmax, "pmax", True), stream_ptr()), "cips3d_to_planes")
    p.cips3d_exp, p.cips3d_pmax = exps, pmax
    return p


def from_planes(p, H, W, out=None):
    lib = _lib.load()
    B, C8 = p.shape[0], p.shape[1]
    x = _given(out, (B, C8 * 8, H, W), torch.float32, p.device, torch.empty)
    exps = getattr(p, "cips3d_exp", None)
    check(lib.cips3d_from_planes(dev_ptr(p, "planes", dtype=torch.float16), dev_ptr(x), B, C8 * 8, H * W,
                                 exps.data_ptr() if exps is not None else None, stream_ptr()), "cips3d_from_planes")
    return x


def modconv1x1_planes(xp, wm_split, Cout, HW, out_format="planes", epilogue=0, noise=None, noise_w=None, bias=None,
                      rgb_w=None, rgb_part=None, demodulated=True, lconst=None, ride=None, half_chip=False, out=None, out_exp=None,
                      out_pmax=None, out_amax=None):
    """1x1 modulated conv on split-fp16 planes (csrc/chain.hip).  xp from to_planes / a previous call (its exponents are read
    from its attribute; a planes output carries its own); wm_split from
    modulate_weights(..., packed=True, split=True).  out_format: "planes" | "fp32" | "bf16" ([B,Cout,HW]).
    demodulated: the weights were demodulated (unit row norm -> the sqrt(Cin) gain of the output bound); for others pass lconst
    from a modulate table that measured the row L1 norms.
    ride: a ToRGB fold carried by this launch (cips3d_reduce_job; range-tracked inputs only) -- dict(part [n_slots, Br, 3, HWr],
    biases [list of [3]], skip [Br, 3, HWr] or None, out [Br, 3, HWr]): out = skip + sum of the slots + sum of the biases, the
    arithmetic and order of torgb_reduce.
    half_chip: cips3d_range.half_chip (another view's launches are in flight: 128 x 128 tiles on half the CUs; same results).
    out / out_exp / out_pmax / out_amax: caller-supplied tensors (the output; the exponents and patch maxima of a range-tracked
    planes output; the amax array, zeroed, that a range-tracked fp32 / bf16 output raises) to write instead of fresh ones."""
    lib = _lib.load()
    B, Cin = xp.shape[0], xp.shape[1] * 8
    dev = xp.device
    fmt = {"fp32": 0, "planes": 1, "bf16": 2}[out_format]
    if fmt == 1:
        out = _given(out, (B, Cout // 8, 2, HW, 8), torch.float16, dev, torch.empty)
    else:
        out = _given(out, (B, Cout, HW), torch.bfloat16 if fmt == 2 else torch.float32, dev, torch.empty)
    nb = HW if (noise is not None and noise.shape[0] == B and B > 1) else 0
    x_exp, x_pmax = getattr(xp, "cips3d_exp", None), getattr(xp, "cips3d_pmax", None)
    ranged = x_exp is not None
    rg, _keep = None, None
    if ranged:
        if lconst is None and fmt == 1:
            if not demodulated:
                raise RuntimeError("a planes output of a non-demodulated conv needs the layer's lconst (row L1 norms)")
            if epilogue == 1:
                lconst = range_consts(B, bias, noise_w, Cin ** 0.5, noise=noise)
            else:
                lconst = range_consts(B, torch.zeros(1, device=dev), None, Cin ** 0.5)
                lconst[:, 1] /= 2.0 ** 0.5      # no activation: |out| <= sqrt(Cin) max|x|
        out_amax = _given(out_amax, (B, amax_floats()), torch.float32, dev, torch.zeros) if fmt != 1 else None
        nblk = (HW + _lib.PLANES_EXP_BLOCK - 1) // _lib.PLANES_EXP_BLOCK
        out_exp = _given(out_exp, (B, nblk), torch.int32, dev, torch.zeros) if fmt == 1 else None
        out_pmax = _given(out_pmax, (B, (HW + 63) // 64, Cout // 16), torch.float32, dev, torch.zeros) if fmt == 1 else None
        # (x_pmax None: the kernel bounds max|in| by what the input's exponent encodes -- looser, still rigorous)
        rg, _keep = _range(x_exp=x_exp, x_pmax=x_pmax if fmt == 1 else None, lconst=lconst if fmt == 1 else None,
                           out_amax=out_amax, out_exp=out_exp, out_pmax=out_pmax)
    job = None
    if ride is not None:
        if rg is None:
            raise RuntimeError("a riding ToRGB fold needs range-tracked input planes (to_planes with x_amax)")
        part, r_out = ride["part"], ride["out"]
        n_slots, Br, _, HWr = part.shape
        job = _lib.ReduceJob()
        job.part, job.out = dev_ptr(part, "ride.part"), dev_ptr(r_out, "ride.out")
        job.skip = dev_ptr(ride.get("skip"), "ride.skip", True)
        for k, bk in enumerate(ride.get("biases", [])):
            job.bias[k] = dev_ptr(bk, "ride.bias")
        job.n4, job.HW4, job.slot_stride = Br * 3 * HWr // 4, HWr // 4, Br * 3 * HWr
        job.n_slots, job.n_bias = n_slots, len(ride.get("biases", []))
        rg.ride = C.addressof(job)
    if rg is not None:
        rg.half_chip = int(bool(half_chip))
    check(lib.cips3d_modconv1x1_planes(dev_ptr(xp, "x_planes", dtype=torch.float16), dev_ptr(wm_split, "wm"), out.data_ptr(), fmt,
                                       B, Cin, Cout, HW, epilogue, dev_ptr(noise, "noise", True), nb,
                                       dev_ptr(noise_w, "noise_w", True), dev_ptr(bias, "bias", True),
                                       dev_ptr(rgb_w, "rgb_w", True), dev_ptr(rgb_part, "rgb_part", True), None,
                                       C.byref(rg) if rg is not None else None, stream_ptr()),
          "cips3d_modconv1x1_planes")
    if ranged:
        if fmt == 1:
            out.cips3d_exp, out.cips3d_pmax = out_exp, out_pmax
        elif fmt == 0:
            tag_amax(out, out_amax)
    return out


def to_planes16(x, out=None):
    """fp32 [B,C,H,W] -> planes16 (torch.bfloat16 tensor [B, C/8, H*W, 8]; round to nearest even)."""
    lib = _lib.load()
    B, Cc, H, W = x.shape
    p = _given(out, (B, Cc // 8, H * W, 8), torch.bfloat16, x.device, torch.empty)
    check(lib.cips3d_to_planes16(dev_ptr(x, "x"), p.data_ptr(), B, Cc, H * W, stream_ptr()), "cips3d_to_planes16")
    return p


def from_planes16(p, H, W, out=None):
    lib = _lib.load()
    B, C8 = p.shape[0], p.shape[1]
    x = _given(out, (B, C8 * 8, H, W), torch.float32, p.device, torch.empty)
    check(lib.cips3d_from_planes16(dev_ptr(p, "planes16", dtype=torch.bfloat16), dev_ptr(x), B, C8 * 8, H * W, stream_ptr()),
          "cips3d_from_planes16")
    return x


def modconv1x1_planes16(xp, wm_bf16, Cout, HW, out_format="planes16", epilogue=0, noise=None, noise_w=None, bias=None,
                        rgb_w=None, rgb_part=None, out=None):
    """1x1 modulated conv of the bf16 decoder mode on planes16 (csrc/chain.hip, NP = 1).  xp from to_planes16 / a previous
    call; wm_bf16 from modulate_weights(..., packed=True, bf16=True).  out_format: "planes16" | "fp32" | "bf16" ([B,Cout,HW]).
    Returns (out, number of rgb_part row-block slots written)."""
    lib = _lib.load()
    B, Cin = xp.shape[0], xp.shape[1] * 8
    fmt = {"fp32": 0, "bf16": 2, "planes16": 3}[out_format]
    if fmt == 3:
        out = _given(out, (B, Cout // 8, HW, 8), torch.bfloat16, xp.device, torch.empty)
    else:
        out = _given(out, (B, Cout, HW), torch.bfloat16 if fmt == 2 else torch.float32, xp.device, torch.empty)
    nb = HW if (noise is not None and noise.shape[0] == B and B > 1) else 0
    nblk = C.c_int(0)
    check(lib.cips3d_modconv1x1_planes16(dev_ptr(xp, "x_planes16", dtype=torch.bfloat16), dev_ptr(wm_bf16, "wm"), out.data_ptr(),
                                         fmt, B, Cin, Cout, HW, epilogue, dev_ptr(noise, "noise", True), nb,
                                         dev_ptr(noise_w, "noise_w", True), dev_ptr(bias, "bias", True),
                                         dev_ptr(rgb_w, "rgb_w", True), dev_ptr(rgb_part, "rgb_part", True), C.byref(nblk),
                                         None, stream_ptr()), "cips3d_modconv1x1_planes16")
    return out, nblk.value


# Fresh noise (NoiseInjection maps, per-ray jitter) from the library's own generator (csrc/rng.hip) in one launch; 0 = torch's
# randn / rand, two launches (A/B knob).  Either way the stream is a function of torch's seed and generator state.
FAST_RNG = os.environ.get("CIPS3D_FAST_RNG", "1") != "0"


def rng_reserve(n_normal, n_uniform, device):
    """(seed, base) of a cips3d_rng_fill draw of these counts taken from torch's generator for `device`, whose Philox offset is
    advanced by what the draw consumes (torch keeps the offset a multiple of 4)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    seed, base = gen.initial_seed(), gen.get_offset()
    threads = int(_lib.load().cips3d_rng_fill_threads(n_normal, n_uniform))
    gen.set_offset(base + 4 * ((threads + 3) // 4))
    return int(seed) & 0xFFFFFFFFFFFFFFFF, int(base)


def rng_fill(n_normal, n_uniform, device, seed=None, base=None):
    """(normal [n_normal] ~ N(0,1), uniform [n_uniform] ~ U[0,1)) fp32 tensors from cips3d_rng_fill (None for a zero count).
    With seed / base omitted the state is torch's: key = the device generator's initial_seed(), counter base = its Philox
    offset, which is advanced by what the call consumes -- torch.manual_seed / get_rng_state / set_rng_state govern this
    stream like torch's own draws."""
    lib = _lib.load()
    device = torch.device(device)
    normal = torch.empty(n_normal, device=device, dtype=torch.float32) if n_normal else None
    uniform = torch.empty(n_uniform, device=device, dtype=torch.float32) if n_uniform else None
    if n_normal == 0 and n_uniform == 0:
        return normal, uniform
    if seed is None:
        seed, base = rng_reserve(n_normal, n_uniform, device)
    check(lib.cips3d_rng_fill(int(seed) & 0xFFFFFFFFFFFFFFFF, int(base), dev_ptr(normal, "normal", True), n_normal,
                              dev_ptr(uniform, "uniform", True), n_uniform, stream_ptr()), "cips3d_rng_fill")
    return normal, uniform


def rng_words(seed, base, n_threads, device):
    """The raw Philox words of threads 0 .. n_threads-1 as an int64 tensor [n_threads, 4] (tests)."""
    out = torch.empty(n_threads, 4, device=device, dtype=torch.int32)
    check(_lib.load().cips3d_rng_words(int(seed) & 0xFFFFFFFFFFFFFFFF, int(base), out.data_ptr(), n_threads, stream_ptr()),
          "cips3d_rng_words")
    return out.to(torch.int64) & 0xFFFFFFFF


def modconv3x3_supported(Cin, Cout, H, W, up):
    return bool(_lib.load().cips3d_modconv3x3_supported(Cin, Cout, H, W, int(bool(up))))


def modconv3x3(x, wm_packed, Cout, up=False, fir=None, epilogue=0, noise=None, noise_w=None, bias=None, split=False, x_amax=None,
               out=None):
    """3x3 modulated conv on the LDS-tiled MFMA kernel (csrc/conv3x3.hip).  x [B,Cin,H,W]; wm_packed from
    modulate_weights(..., ksq=9, packed=True, flip=up); up: conv_transpose2d(stride 2) + Blur(fir) fused -> [B,Cout,2H,2W].
    split: fp32-equivalent split-fp16 products (wm_packed from modulate_weights(..., split=True) as well); x is split as x * 2^-e
    from its measured maximum (x_amax: its amax array, else the one attached to x, else measured here)."""
    lib = _lib.load()
    B, Cin, H, W = x.shape
    OH, OW = (2 * H, 2 * W) if up else (H, W)
    if out is None:
        out = torch.empty(B, Cout, OH, OW, device=x.device, dtype=torch.float32)
    nb = 0
    if noise is not None:
        if noise.shape[0] not in (1, B) or tuple(noise.shape[-2:]) != (OH, OW):
            raise RuntimeError(f"noise must be (1|{B},1,{OH},{OW}), got {tuple(noise.shape)}")
        nb = OH * OW if (noise.shape[0] == B and B > 1) else 0
    rg, _keep = None, None
    if split:
        rg, _keep = _range(x_amax=x_amax if x_amax is not None else amax_of(x))
    check(lib.cips3d_modconv3x3(dev_ptr(x, "x"), dev_ptr(wm_packed, "wm"), dev_ptr(out), B, Cin, Cout, H, W, int(bool(up)),
                                dev_ptr(fir, "fir", True), int(epilogue) | (GEMM_SPLIT if split else 0), dev_ptr(noise, "noise", True), nb,
                                dev_ptr(noise_w, "noise_w", True), dev_ptr(bias, "bias", True),
                                C.byref(rg) if rg is not None else None, stream_ptr()),
          "cips3d_modconv3x3")
    return out


def fused_up_conv_chains(C_):
    return bool(_lib.load().cips3d_fused_up_conv_chains(C_))


def fused_up_conv(y_lo, fir, noise1, noise_w1, bias1, wm2_packed, noise2, noise_w2, bias2, wm_rgb=None, bias_rgb=None,
                  skip=None, skip_up=True, want_out2=True, bf16=False, wm_next=None, split=False, ranged=True, flat=False,
                  rgb_u8=False, out=None):
    """FIR up-sampling + act -> 1x1 conv + act -> ToRGB for one up-sampling stage (see cips3d_fused_up_conv).
    wm_next (MOD_PACKED | MOD_CHAINED weights of the next stage's C -> C/2 up-conv): also returns its low-res GEMM y_next.
    A torch.bfloat16 `y_lo` selects the bf16-storage form (CIPS3D_Y_BF16, needs bf16=True): y_next is then bf16 as well.
    split: fp32-equivalent split-fp16 products; wm2_packed / wm_next must then be MOD_SPLIT16-packed.  The stage's operands are
    then split under power-of-two scales from rigorous bounds (cips3d_range): y_lo's amax array is taken from its tag or
    measured, the two layers' constants are made here (noise bounds measured on the device); out2 / y_next leave tagged.
    flat: a block that does not up-sample (CIPS3D_STAGE_FLAT): y_lo is conv1's GEMM result at the block's resolution, fir is
    not read, outputs and skip have y_lo's size (skip_up must be False).
    rgb_u8: the image leaves as a torch.uint8 tensor (CIPS3D_RGB_U8).  out: (out2, rgb, y_next), contiguous tensors of the shapes
    and dtypes this function would allocate, to write into; an entry that is None is allocated here."""
    lib = _lib.load()
    B, Cc, H, W = y_lo.shape
    up = 1 if flat else 2
    if flat:
        skip_up = False          # (the skip image of a flat stage has the output's size and is added as it is)
    rg, _keep, next_amax = None, None, None
    if split and ranged:
        lc1 = range_consts(B, bias1, noise_w1, 0.0, fir=fir, noise=noise1)
        lc2 = range_consts(B, bias2, noise_w2, Cc ** 0.5, noise=noise2)
        next_amax = new_amax(B, y_lo.device) if wm_next is not None else None
        rg, _keep = _range(x_amax=amax_of(y_lo), lconst=lc1, lconst2=lc2, next_amax=next_amax)
    dev = y_lo.device
    ydt = y_lo.dtype
    if ydt == torch.bfloat16 and not bf16:
        raise RuntimeError("a bf16 y_lo needs the bf16 GEMM mode (bf16=True)")
    rdt = torch.uint8 if rgb_u8 else torch.float32

    def result(given, wanted, ch, dtype, name):
        if not wanted:
            return None
        if given is None:
            return torch.empty(B, ch, up * H, up * W, device=dev, dtype=dtype)
        if given.shape != (B, ch, up * H, up * W) or given.device != dev:
            raise RuntimeError(f"fused_up_conv: `out` {name} must be [{B}, {ch}, {up * H}, {up * W}] on {dev}")
        return given

    o2, orgb, onext = out if out is not None else (None, None, None)
    out2 = result(o2, want_out2, Cc, torch.float32, "out2")
    rgb = result(orgb, wm_rgb is not None, 3, rdt, "rgb")
    y_next = result(onext, wm_next is not None, Cc // 2, ydt, "y_next")

    def bs(nz):
        return up * up * H * W if (nz is not None and nz.shape[0] == B and B > 1) else 0

    check(lib.cips3d_fused_up_conv_next(dev_ptr(y_lo, "y_lo", dtype=ydt), dev_ptr(fir, "fir", flat), dev_ptr(noise1, "noise1", True), bs(noise1),
                                        dev_ptr(noise_w1, "noise_w1", True), dev_ptr(bias1, "bias1"), dev_ptr(wm2_packed, "wm2"),
                                        dev_ptr(noise2, "noise2", True), bs(noise2), dev_ptr(noise_w2, "noise_w2", True),
                                        dev_ptr(bias2, "bias2"), dev_ptr(out2, "out2", True), dev_ptr(wm_rgb, "wm_rgb", True),
                                        dev_ptr(bias_rgb, "bias_rgb", True), dev_ptr(skip, "skip", True),
                                        int(bool(skip_up)) | (GEMM_BF16 if bf16 else 0) |
                                        (Y_BF16 if ydt == torch.bfloat16 else 0) | (GEMM_SPLIT if split else 0) | (STAGE_FLAT if flat else 0) |
                                        (RGB_U8 if rgb_u8 else 0),
                                        dev_ptr(rgb, "rgb", True, dtype=rdt), dev_ptr(wm_next, "wm_next", True),
                                        dev_ptr(y_next, "y_next", True, dtype=ydt), B, Cc, H, W,
                                        C.byref(rg) if rg is not None else None, stream_ptr()), "cips3d_fused_up_conv_next")
    if next_amax is not None:
        tag_amax(y_next, next_amax)
    if wm_next is not None:
        return out2, rgb, y_next
    return out2, rgb


def rgb_to_uint8(rgb, out=None):
    """[-1,1] float image -> uint8 (clamp, scale, round to nearest) on the device; `out`: a contiguous uint8 tensor of the
    same shape to write into (a slice of a sequence's frame buffer: multiview.sample_multi_view)."""
    lib = _lib.load()
    x = rgb.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
        raise RuntimeError("rgb_to_uint8: `out` must be a contiguous uint8 tensor of the input's shape on its device")
    check(lib.cips3d_rgb_to_uint8(dev_ptr(x, "rgb"), out.data_ptr(), x.numel(), stream_ptr()), "cips3d_rgb_to_uint8")
    return out


# ---------------------------------------------------------------------------------------------- backward entry points
def linear_bwd(x, W, dout, out=None, w_scale=1.0, b_scale=1.0, lrelu=False, act_gain=1.0, out_scale=1.0, need_dx=True,
               need_dW=True, need_db=True):
    lib = _lib.load()
    B, in_dim = x.shape
    out_dim = W.shape[0]
    dev = x.device
    dx = torch.empty(B, in_dim, device=dev) if need_dx else None
    dW = torch.empty(out_dim, in_dim, device=dev) if need_dW else None
    db = torch.empty(out_dim, device=dev) if need_db else None
    check(lib.cips3d_linear_bwd(dev_ptr(x, "x"), x.stride(0), dev_ptr(W, "W"), dev_ptr(out, "out", True),
                                out.stride(0) if out is not None else 0, dev_ptr(dout, "dout"), dout.stride(0), B, in_dim,
                                out_dim, w_scale, b_scale, int(lrelu), act_gain, out_scale, dev_ptr(dx, "dx", True), in_dim,
                                dev_ptr(dW, "dW", True), dev_ptr(db, "db", True), stream_ptr()), "cips3d_linear_bwd")
    return dx, dW, db


def modulate_bwd(dwm, W, s, Cout, Cin, ksq, scale, demodulate, need_dW=True):
    """dwm [B,Cout,Cin*ksq] is consumed (scratch).  Returns (dW shaped like W or None, ds [B,Cin])."""
    lib = _lib.load()
    B = s.shape[0]
    dW = torch.empty_like(W) if need_dW else None
    ds = torch.empty(B, Cin, device=W.device)
    check(lib.cips3d_modulate_bwd(dev_ptr(dwm, "dwm"), dev_ptr(W, "W"), dev_ptr(s, "s"), s.stride(0), B, Cout, Cin, ksq,
                                  float(scale), int(bool(demodulate)), dev_ptr(dW, "dW", True), dev_ptr(ds), Cin, stream_ptr()),
          "cips3d_modulate_bwd")
    return dW, ds


# The GEMMs of the differentiable path whose B operand is an ACTIVATION (decoder forward, the materialised NeRF recompute) run
# in the fp32-equivalent split-fp16 mode, as the inference forward's stand-alone GEMMs do; 0 = the fp32 MFMA (A/B knob).  The
# data-gradient GEMMs keep the fp32 MFMA: their B operand is a gradient tensor whose scale is arbitrary (1e-6 and below), and
# the fp16 halves of the split have an absolute floor of 2^-25 -- fine for O(1) activations, 5 bits for a 1e-6 gradient.
SPLIT_BACKWARD = os.environ.get("CIPS3D_SPLIT_BACKWARD", "1") != "0"


def pack_weights(wm, transpose=False, split=False):
    """wm [B,M,K] -> packed A fragments of wm (or of wm^T); split: fp16 hi + lo fragments for modconv1x1(split=True)."""
    lib = _lib.load()
    B, M, K = wm.shape
    out = torch.empty(B * M * K, device=wm.device)
    check(lib.cips3d_pack_weights(dev_ptr(wm, "wm"), dev_ptr(out), B, M, K, int(bool(transpose)) | (2 if split else 0),
                                  stream_ptr()), "cips3d_pack_weights")
    return out


def gemm_wgrad(dy, x):
    """dy [B,M,...], x [B,K,...] (same trailing pixels) -> dwm [B,M,K]."""
    lib = _lib.load()
    B, M = dy.shape[:2]
    K = x.shape[1]
    P = dy[0, 0].numel()
    dwm = torch.empty(B, M, K, device=dy.device)
    check(lib.cips3d_gemm_wgrad(dev_ptr(dy, "dy"), dev_ptr(x, "x"), dev_ptr(dwm), B, M, K, P, stream_ptr()), "cips3d_gemm_wgrad")
    return dwm


def modconv1x1_actbwd(g, wm_t_packed, y, noise=None, rgb_w=None, drgb=None, split=False, g_amax=None, d_bias=None,
                      d_noise_w=None, d_rgb_w=None, track=True):
    """The data-gradient GEMM with the previous layer's activation backward as its epilogue (cips3d_modconv1x1_actbwd):
    g [B,Cin,H,W], wm_t_packed = pack of wm^T [B,Cout,Cin], y [B,Cout,H,W] the previous layer's stored output -> dpre
    [B,Cout,H,W]; the given accumulators (zeroed by the caller) are added to.  Returns (dpre, amax array of dpre or None)."""
    lib = _lib.load()
    B, Cin, H, W = g.shape
    Cout = y.shape[1]
    out = torch.empty_like(y)
    out_amax = new_amax(B, g.device) if track else None
    rg, _keep = _range(x_amax=g_amax if split else None, out_amax=out_amax)
    ab = _lib.ActBwd()
    ab.y, ab.rgb_w, ab.drgb = dev_ptr(y, "y"), dev_ptr(rgb_w, "rgb_w", True), dev_ptr(drgb, "drgb", True)
    ab.d_bias, ab.d_noise_w, ab.d_rgb_w = dev_ptr(d_bias, "d_bias", True), dev_ptr(d_noise_w, "d_noise_w", True), dev_ptr(d_rgb_w, "d_rgb_w", True)
    nb = H * W if (noise is not None and noise.shape[0] == B and B > 1) else 0
    check(lib.cips3d_modconv1x1_actbwd(dev_ptr(g, "g"), dev_ptr(wm_t_packed, "wm_t"), dev_ptr(out), B, Cin, Cout, H * W,
                                       GEMM_SPLIT if split else 0, C.byref(ab), dev_ptr(noise, "noise", True), nb, C.byref(rg),
                                       stream_ptr()), "cips3d_modconv1x1_actbwd")
    return out, out_amax


def gemm_wgrad_split(dy, x, dy_amax=None, x_amax=None, out=None):
    """gemm_wgrad on split-fp16 products; dy_amax / x_amax: per-sample amax slot arrays (new_amax / absmax) or None.
    out: accumulate into this [B,M,K] tensor instead of returning a fresh one."""
    lib = _lib.load()
    B, M = dy.shape[:2]
    K = x.shape[1]
    P = dy[0, 0].numel()
    dwm = out if out is not None else torch.empty(B, M, K, device=dy.device)
    check(lib.cips3d_gemm_wgrad_split(dev_ptr(dy, "dy"), dev_ptr(x, "x"), dev_ptr(dwm), B, M, K, P, dev_ptr(dy_amax, "dy_amax", True),
                                      dev_ptr(x_amax, "x_amax", True), 1 if out is not None else 0, stream_ptr()),
          "cips3d_gemm_wgrad_split")
    return dwm


def noise_bias_act_bwd(dy, y, noise, noise_w, need_dnoise=False, need_dnw=True, need_db=True):
    lib = _lib.load()
    B, Cc = y.shape[:2]
    HW = y[0, 0].numel()
    dev = y.device
    dx = torch.empty_like(y)
    nb = HW if (noise is not None and noise.shape[0] == B and B > 1) else 0
    dnoise = torch.empty_like(noise) if (need_dnoise and noise is not None) else None
    dnw = torch.empty(1, device=dev) if (need_dnw and noise is not None) else None
    if need_db and dnw is not None:       # back to back: the library zeroes both with one memset
        both = torch.empty(2 * Cc, device=dev)
        db, scratch = both[:Cc], both[Cc:]
    else:
        db = torch.empty(Cc, device=dev) if need_db else None
        scratch = torch.empty(Cc, device=dev) if dnw is not None else None
    check(lib.cips3d_noise_bias_act_bwd(dev_ptr(dy, "dy"), dev_ptr(y, "y"), dev_ptr(noise, "noise", True), nb,
                                        dev_ptr(noise_w, "noise_w", True), dev_ptr(dx), dev_ptr(dnoise, "dnoise", True),
                                        dev_ptr(dnw, "dnw", True), dev_ptr(db, "db", True), dev_ptr(scratch, "scratch", True),
                                        B, Cc, HW, stream_ptr()),
          "cips3d_noise_bias_act_bwd")
    return dx, dnoise, dnw, db


def torgb_bwd(drgb, x, wm, need_db=True):
    lib = _lib.load()
    B, Cc = x.shape[:2]
    HW = x[0, 0].numel()
    dx = torch.empty_like(x)
    both = torch.empty(B * 3 * Cc + 3, device=x.device)      # dwm and dbias back to back: one memset in the library
    dwm = both[:B * 3 * Cc].view(B, 3, Cc)
    db = both[B * 3 * Cc:] if need_db else None
    check(lib.cips3d_torgb_bwd(dev_ptr(drgb, "drgb"), dev_ptr(x, "x"), dev_ptr(wm, "wm"), dev_ptr(dx), dev_ptr(dwm),
                               dev_ptr(db, "db", True), B, Cc, HW, stream_ptr()), "cips3d_torgb_bwd")
    return dx, dwm, db


def camera_params_bwd(locations, dextr, up=None):
    lib = _lib.load()
    B = locations.shape[0]
    loc = locations.detach().float().contiguous()
    up_t = up.detach().float().contiguous() if up is not None else None
    dloc = torch.empty(B, 2, device=loc.device)
    dextr = dextr.contiguous()
    check(lib.cips3d_camera_params_bwd(dev_ptr(loc, "locations"), dev_ptr(up_t, "up", True), dev_ptr(dextr, "dextr"),
                                       B, dev_ptr(dloc), stream_ptr()), "cips3d_camera_params_bwd")
    return dloc


def _geo_upstreams(d_mask, d_xyz, xyz, B, R):
    """The upstreams of the render's geometry maps as the kernels take them: d_mask [2,B,S,S] (planar: d mask[0], d depth), d_xyz
    [B,3,S,S] and the forward's xyz [B,3,S,S] -> contiguous fp32 (d_mask [2,B,R] | None, d_xyz [B,3,R] | None, xyz | None)."""
    if d_mask is not None and xyz is None:
        raise ValueError("d_mask needs xyz, the forward's map: the depth channel is -|xyz|")
    if d_mask is None and d_xyz is None:
        return None, None, None
    dm = None if d_mask is None else d_mask.float().reshape(2, B, R).contiguous()
    dx = None if d_xyz is None else d_xyz.float().reshape(B, 3, R).contiguous()
    return dm, dx, None if dm is None else xyz.detach().float().reshape(B, 3, R).contiguous()


def _nerf_bwd_geom(cam_poses, focals, near, far, perturb_u, img_size, n_samples, static_viewdirs, into=None):
    """The NerfBwdGeom (cips3d_nerf_bwd_geom) of both NeRF backwards, a new one or `into` filled: returns (geom, the tensors it
    points into, which the caller holds until its calls are enqueued)."""
    geom = _lib.NerfBwdGeom() if into is None else into
    B, R = cam_poses.shape[0], img_size * img_size
    keep = [cam_poses.float().contiguous(), focals.float().reshape(B).contiguous(), near.float().reshape(B).contiguous(),
            far.float().reshape(B).contiguous(),
            None if perturb_u is None else perturb_u.float().reshape(B, R).contiguous()]
    geom.cam_poses, geom.focals, geom.near_, geom.far_ = (dev_ptr(t) for t in keep[:4])
    geom.perturb_u = dev_ptr(keep[4], "perturb_u", True)
    geom.B, geom.img_size, geom.n_samples, geom.static_viewdirs = B, img_size, n_samples, int(bool(static_viewdirs))
    return geom, keep


def nerf_backward(net, sigmoid_beta, cam_poses, focals, near, far, perturb_u, film, layer_bias, img_size, n_samples,
                  static_viewdirs, d_features, d_thumb, need_params=False, d_mask=None, d_xyz=None, xyz=None, d_focal=False):
    """The materialised NeRF backward (see csrc/nerf_bwd.hip): returns (dfilm [B,L,2,H], dcam [B,3,4]) -- and, with
    need_params (`optim_render_params`, models/projector_v10.py:848-872), a dict of the gradients of the renderer's own
    weights: pts_linears.{l}.weight / .bias, views_linears.weight / .bias, rgb_linear.*, sigma_linear.*, sigmoid_beta
    (the gamma / beta heads get theirs from the FiLM table's backward).

    net = SirenGenerator (weights), film [B,L,2,H], layer_bias [L,H]; d_features [B,H,S,S], d_thumb [B,3,S,S].
    d_mask [2,B,S,S] (d mask[0], d depth) and d_xyz [B,3,S,S]: the upstreams of the geometry maps, None = absent; d_mask needs
    `xyz`, the forward's [B,3,S,S] map.  They enter the compositing backward and the camera chain -- no further launch.
    d_focal=True (opt-in): d loss / d focals [B] is appended to the returned tuple -- the camera chain's second instantiation
    (cips3d_nerf_bwd_camera with dfocal) and one [B] memset; False launches exactly what it did without the argument."""
    lib = _lib.load()
    st = stream_ptr()
    dev = cam_poses.device
    B = cam_poses.shape[0]
    H = net.W
    D = net.D
    L = D + 1
    R = img_size * img_size
    P = R * n_samples
    fb = L * 2 * H
    geom, keep = _nerf_bwd_geom(cam_poses, focals, near, far, perturb_u, img_size, n_samples, static_viewdirs)
    gp = C.byref(geom)
    new = lambda *shape: torch.empty(*shape, device=dev)
    film = film.contiguous()
    film_l = lambda l: film.data_ptr() + 4 * (l * 2 * H)

    # ---- forward recompute
    ptsn, viewdirs = new(B, 3, P), new(B, 3, R)
    pre = [new(B, H, P)] + [None] * (L - 1)
    hh = [new(B, H, P) for _ in range(L)]
    w_first = net.pts_linears[0].weight
    check(lib.cips3d_nerf_bwd_points(gp, dev_ptr(w_first), layer_bias.data_ptr(), film_l(0), fb, H, dev_ptr(ptsn),
                                     dev_ptr(pre[0]), dev_ptr(hh[0]), dev_ptr(viewdirs), st), "cips3d_nerf_bwd_points")
    w_view = net.views_linears.weight                      # [H, H+3]
    mats = [net.pts_linears[l].weight.detach() for l in range(1, D)] + [w_view.detach()[:, :H].contiguous()]
    split = SPLIT_BACKWARD and H % 32 == 0
    packed, packed_t = [], []
    for Wl in mats:                                        # shared over the batch: replicate the (small) matrix
        Wb = Wl.unsqueeze(0).expand(B, H, H).contiguous()
        packed.append(pack_weights(Wb, split=split))            # forward recompute: activations in [-1, 1]
        packed_t.append(pack_weights(Wb, transpose=True))       # data gradients: fp32 MFMA (see SPLIT_BACKWARD)

    sine_amax = const_amax(B, 1.0, dev)         # the recompute's GEMM inputs are FiLM sines

    def gemm(x, pk, sp=False):
        return modconv1x1(x.view(B, H, P, 1), pk, H, epilogue=0, split=sp, x_amax=sine_amax, track=False).view(B, H, P)

    for l in range(1, L):
        acc = gemm(hh[l - 1], packed[l - 1], split)
        is_view = l == D
        check(lib.cips3d_nerf_bwd_film(dev_ptr(acc), dev_ptr(hh[l]), layer_bias.data_ptr() + 4 * l * H, film_l(l), fb,
                                       (w_view.data_ptr() + 4 * H) if is_view else None, H + 3,
                                       dev_ptr(viewdirs) if is_view else None, B, H, R, P, st), "cips3d_nerf_bwd_film")
        pre[l] = acc
    h_last, f = hh[D - 1], hh[D]
    sdf, crgb, g = new(B, 1, P), new(B, 3, P), new(B, P)
    check(lib.cips3d_nerf_bwd_heads(dev_ptr(h_last), dev_ptr(net.sigma_linear.weight), H, 1, dev_ptr(net.sigma_linear.bias), 1,
                                    B, H, P, dev_ptr(sdf), st), "cips3d_nerf_bwd_heads")
    check(lib.cips3d_nerf_bwd_heads(dev_ptr(f), dev_ptr(net.rgb_linear.weight), H, 1, dev_ptr(net.rgb_linear.bias), 3, B, H, P,
                                    dev_ptr(crgb), st), "cips3d_nerf_bwd_heads")
    dF = d_features.contiguous().view(B, H, R)
    dth = d_thumb.contiguous().view(B, 3, R)
    check(lib.cips3d_nerf_bwd_dot(dev_ptr(dF), dev_ptr(f), B, H, R, P, dev_ptr(g), st), "cips3d_nerf_bwd_dot")

    # ---- compositing backward
    wts, Tb, dsdf, dcrgb, ddnorm = new(B, P), new(B, P), new(B, P), new(B, 3, P), new(B, R)
    dbeta_ray = new(B, R) if need_params else None
    dm, dx, xm = _geo_upstreams(d_mask, d_xyz, xyz, B, R)
    geo = dm is not None or dx is not None
    wsum, wzsum = (new(B, R), new(B, R)) if geo else (None, None)
    geo_ptrs = (dev_ptr(dm, "d_mask", True), dev_ptr(dx, "d_xyz", True), dev_ptr(xm, "xyz", True),
                dev_ptr(wsum, "wsum", True), dev_ptr(wzsum, "wzsum", True))
    check(lib.cips3d_nerf_bwd_composite(gp, dev_ptr(sdf), dev_ptr(crgb), dev_ptr(g), dev_ptr(dth),
                                        dev_ptr(sigmoid_beta, "sigmoid_beta", True),      # None: with_sdf = False
                                        dev_ptr(wts), dev_ptr(Tb), dev_ptr(dsdf), dev_ptr(dcrgb), dev_ptr(ddnorm),
                                        dev_ptr(dbeta_ray, "dbeta_ray", True), *geo_ptrs, st), "cips3d_nerf_bwd_composite")

    # ---- gradients of the renderer's own weights (optional): the wide blocks W_l [H,H] on the split-fp16 weight-gradient
    # GEMM (contraction over the points), everything narrow -- biases, the first layer, the view-direction columns, the heads
    # -- as row dots
    pg = {}

    def row_dots(a, rows, Pa, x=None, nx=0, Px=0):
        out = torch.zeros(rows, 4, device=dev)
        check(lib.cips3d_nerf_bwd_row_dots(dev_ptr(a), dev_ptr(x, "x", True), nx, Px, dev_ptr(out), B, rows, Pa, st),
              "cips3d_nerf_bwd_row_dots")
        return out

    def wide(dp, h):                 # sum_b dp[b] h[b]^T
        if H % 32 or P % 32:
            return gemm_wgrad(dp, h).sum(0)
        acc = torch.zeros(1, H, H, device=dev)
        am = absmax(dp)
        for b in range(B):
            gemm_wgrad_split(dp[b:b + 1], h[b:b + 1], am[b:b + 1], sine_amax[:1], out=acc)
        return acc[0]

    if need_params:
        t = row_dots(f, H, P, dcrgb, 3, P)
        pg["rgb_linear.weight"] = t[:, :3].t().contiguous()
        pg["rgb_linear.bias"] = row_dots(dcrgb, 3, P)[:, 3].contiguous()
        pg["sigma_linear.weight"] = row_dots(h_last, H, P, dsdf, 1, P)[:, :1].t().contiguous()
        pg["sigma_linear.bias"] = row_dots(dsdf, 1, P)[:, 3].contiguous()
        pg["sigmoid_beta"] = row_dots(dbeta_ray, 1, R)[:, 3].contiguous() if sigmoid_beta is not None else torch.zeros(1, device=dev)

    # ---- MLP backward
    dfilm = torch.zeros(B, L, 2, H, device=dev)
    dfilm_l = lambda l: dfilm.data_ptr() + 4 * (l * 2 * H)
    check(lib.cips3d_nerf_bwd_film_grad(dev_ptr(f), dev_ptr(pre[D]), film_l(D), fb, 1, None, None, dev_ptr(wts), dev_ptr(dF),
                                        dev_ptr(net.rgb_linear.weight), dev_ptr(dcrgb), dfilm_l(D), B, H, R, P, st),
          "cips3d_nerf_bwd_film_grad")
    dpre = f
    dvd_pt = new(B, 3, P)
    check(lib.cips3d_nerf_bwd_heads(dev_ptr(dpre), w_view.data_ptr() + 4 * H, 1, H + 3, None, 3, B, H, P, dev_ptr(dvd_pt), st),
          "cips3d_nerf_bwd_heads")
    if need_params:                                        # the view layer: [h_{D-1} | view direction] -> H
        t = row_dots(dpre, H, P, viewdirs, 3, R)
        pg["views_linears.weight"] = torch.cat([wide(dpre, hh[D - 1]), t[:, :3]], 1)
        pg["views_linears.bias"] = t[:, 3].contiguous()
    for l in range(D, 0, -1):
        dh = gemm(dpre, packed_t[l - 1])                  # gradient w.r.t. h_{l-1}
        first = l == D                                     # h_{D-1} also feeds the sigma head
        check(lib.cips3d_nerf_bwd_film_grad(dev_ptr(dh), dev_ptr(pre[l - 1]), film_l(l - 1), fb, 0,
                                            dev_ptr(net.sigma_linear.weight) if first else None,
                                            dev_ptr(dsdf) if first else None, None, None, None, None, dfilm_l(l - 1), B, H, R,
                                            P, st), "cips3d_nerf_bwd_film_grad")
        dpre = dh                                          # now d(pre_{l-1})
        if need_params:
            if l - 1 >= 1:
                pg[f"pts_linears.{l - 1}.weight"] = wide(dpre, hh[l - 2])
                pg[f"pts_linears.{l - 1}.bias"] = row_dots(dpre, H, P)[:, 3].contiguous()
            else:
                t = row_dots(dpre, H, P, ptsn, 3, P)
                pg["pts_linears.0.weight"] = t[:, :3].contiguous()
                pg["pts_linears.0.bias"] = t[:, 3].contiguous()
    dptsn = new(B, 3, P)
    check(lib.cips3d_nerf_bwd_heads(dev_ptr(dpre), dev_ptr(w_first), 1, 3, None, 3, B, H, P, dev_ptr(dptsn), st),
          "cips3d_nerf_bwd_heads")
    dcam = new(B, 3, 4)
    dfoc = torch.zeros(B, device=dev) if d_focal else None
    check(lib.cips3d_nerf_bwd_camera(gp, dev_ptr(dptsn), dev_ptr(dvd_pt), dev_ptr(ddnorm), *geo_ptrs, 0, dev_ptr(dcam),
                                     dev_ptr(dfoc, "dfocal", True), st), "cips3d_nerf_bwd_camera")
    out = (dfilm, dcam, pg) if need_params else (dfilm, dcam)
    return out + (dfoc,) if d_focal else out


def nerf_pack_weights_t(w_hidden, w_view, packed, hidden, depth):
    """The transposed weight stream of the fused NeRF backward (consumption order, forward scales; cips3d_nerf_pack_weights_t)."""
    lib = _lib.load()
    packed_t = torch.empty_like(packed)
    check(lib.cips3d_nerf_pack_weights_t(dev_ptr(w_hidden, "w_hidden", True), dev_ptr(w_view, "w_view"), dev_ptr(packed),
                                         dev_ptr(packed_t), hidden, depth, stream_ptr()), "cips3d_nerf_pack_weights_t")
    return packed_t


FUSED_NERF_BACKWARD = os.environ.get("CIPS3D_FUSED_NERF_BACKWARD", "1") != "0"   # A/B knob: 0 = the materialised sequence
STASH_IN_FORWARD = os.environ.get("CIPS3D_STASH_IN_FORWARD", "1") != "0"         # A/B knob: 0 = the backward recomputes the forward


def nerf_backward_fused_supported(hidden, depth, img_size, n_samples):
    return bool(_lib.load().cips3d_nerf_bwd_fused_supported(hidden, depth, img_size, n_samples))


def nerf_forward_stash(B, img_size, n_samples, hidden, depth, device, n_chunks=None):
    """Buffers a differentiable forward hands to cips3d_nerf_render (`stash`, `bwd_sdf`, `bwd_crgb`) and later, as `fwd`, to
    nerf_backward_fused: dict(stash, sdf, crgb, n_chunks)."""
    lib = _lib.load()
    if n_chunks is None:
        n_chunks = nerf_suggest_chunks(B, img_size, n_samples)
    P = img_size * img_size * n_samples
    return {"stash": torch.empty(int(lib.cips3d_nerf_bwd_fused_stash_floats(B, img_size, n_samples, hidden, depth, n_chunks)),
                                 device=device),
            "sdf": torch.empty(B, P, device=device), "crgb": torch.empty(B, 3, P, device=device), "n_chunks": n_chunks}


def nerf_backward_fused(net, sigmoid_beta, cam_poses, focals, near, far, perturb_u, film, layer_bias, packed, packed_t, img_size,
                        n_samples, static_viewdirs, d_features, d_thumb, fwd=None, d_mask=None, d_xyz=None, xyz=None, n_chunks=None,
                        stash=None, d_focal=False):
    """The fused NeRF backward (csrc/nerf_bwd_fused.hip): returns (dfilm [B,L,2,H], dcam [B,3,4]); same contract as
    nerf_backward (d_mask / d_xyz / xyz and the opt-in d_focal, which appends d loss / d focals [B], included).  `fwd` = the nerf_forward_stash buffers a differentiable forward filled: the
    forward is then not recomputed.  `n_chunks` (without `fwd`, which carries its own): chunks a ray's samples are split into,
    1 .. n_samples; None = nerf_suggest_chunks.  `stash` (without `fwd`): a float32 buffer of cips3d_nerf_bwd_fused_stash_floats
    floats that the forward recompute fills instead of a private allocation."""
    lib = _lib.load()
    dev = cam_poses.device
    B, H, D = cam_poses.shape[0], net.W, net.D
    L, R = D + 1, img_size * img_size
    p = _lib.NerfBwdFusedParams()
    _, keep = _nerf_bwd_geom(cam_poses, focals, near, far, perturb_u, img_size, n_samples, static_viewdirs, into=p.geom)
    keep += [film.float().contiguous(), d_features.float().contiguous(), d_thumb.float().contiguous()]
    if fwd is not None:
        if stash is not None:
            raise ValueError("stash= is the recompute route's buffer: with fwd= the forward's own stash is read")
        if n_chunks is not None and int(n_chunks) != fwd["n_chunks"]:
            raise ValueError(f"n_chunks = {n_chunks}, but the forward filled its stash for {fwd['n_chunks']} chunks")
        n_chunks, stash = fwd["n_chunks"], fwd["stash"]
        p.fwd_sdf, p.fwd_crgb = dev_ptr(fwd["sdf"]), dev_ptr(fwd["crgb"])
    else:
        if n_chunks is None:
            n_chunks = nerf_suggest_chunks(B, img_size, n_samples)
        n_chunks = int(n_chunks)
        if not 1 <= n_chunks <= n_samples:
            raise ValueError(f"n_chunks = {n_chunks}: must lie in 1 .. n_samples = {n_samples}")
        n_stash = int(lib.cips3d_nerf_bwd_fused_stash_floats(B, img_size, n_samples, H, D, n_chunks))
        if stash is None:
            stash = torch.empty(n_stash, device=dev)
        elif stash.dtype != torch.float32 or stash.device != dev or not stash.is_contiguous() or stash.numel() != n_stash:
            raise ValueError(f"stash: a contiguous float32 buffer of {n_stash} floats on {dev} is needed")
    scratch = torch.empty(int(lib.cips3d_nerf_bwd_fused_scratch_floats(B, img_size, n_samples, H, D)), device=dev)
    dfilm, dcam = torch.empty(B, L, 2, H, device=dev), torch.empty(B, 3, 4, device=dev)
    p.w_first, p.packed, p.packed_t = dev_ptr(net.pts_linears[0].weight), dev_ptr(packed), dev_ptr(packed_t)
    p.w_view, p.film, p.layer_bias = dev_ptr(net.views_linears.weight), dev_ptr(keep[5]), dev_ptr(layer_bias)
    p.w_sigma, p.b_sigma = dev_ptr(net.sigma_linear.weight), dev_ptr(net.sigma_linear.bias)
    p.w_rgb, p.b_rgb = dev_ptr(net.rgb_linear.weight), dev_ptr(net.rgb_linear.bias)
    p.sigmoid_beta = dev_ptr(sigmoid_beta, "sigmoid_beta", True)      # None: with_sdf = False (raw density)
    p.d_features, p.d_thumb = dev_ptr(keep[6]), dev_ptr(keep[7])
    p.stash, p.scratch, p.dfilm, p.dcam = dev_ptr(stash), dev_ptr(scratch), dev_ptr(dfilm), dev_ptr(dcam)
    p.hidden, p.depth, p.n_chunks = H, D, n_chunks
    geo = _geo_upstreams(d_mask, d_xyz, xyz, B, R)          # (held until the call is enqueued)
    p.d_mask, p.d_xyz, p.xyz = (dev_ptr(t, "geometry upstream", True) for t in geo)
    dfoc = torch.empty(B, device=dev) if d_focal else None  # (cleared by the call)
    check(lib.cips3d_nerf_bwd_fused(C.byref(p), dev_ptr(dfoc, "dfocal", True), stream_ptr()), "cips3d_nerf_bwd_fused")
    return (dfilm, dcam, dfoc) if d_focal else (dfilm, dcam)


def inversion_roofline(renderer, B, n_samples, img_size=64, iters=10):
    """Roofline entry of the flip-inversion step's dominant piece: the fused NeRF backward (csrc/nerf_bwd_fused.hip:
    nerf_stash_kernel + nerf_bwd_kernel, ~23 % of the step), timed stand-alone on the step's shape with HIP events around
    cips3d_nerf_bwd_fused (the three per-ray / preparation kernels inside the call are ~4 % of it).  Algorithmic flop = the
    forward point MLP once more + the data-gradient GEMMs W_l^T d(pre_l); executed as split-fp16 products, so the peak is the
    fp16 dense MFMA peak / 3 (as for the forward render kernel)."""
    from . import autograd as AG
    from .camera import Camera
    dev = "cuda"
    net = renderer.network
    H, D, S = net.W, net.D, img_size
    locs = torch.tensor([[0.25, 0.1], [-0.25, 0.1]] * ((B + 1) // 2))[:B].to(dev)
    cam, focal, near, far = Camera.generate_camera_params(locations=locs, img_size=S, device=dev, fov_ang=15,
                                                          dist_radius=0.3)[:4]
    from . import weights
    styles = (0.5 * weights.det_normal("roofline.styles", (B, D + 1, renderer.style_dim), 1.0, 1)).to(dev)
    film = AG.film_table(renderer, styles).detach()
    u = weights.det_unit_uniform("roofline.u", (B, S, S, 1), 2).to(dev)
    dF = (1e-5 * weights.det_normal("roofline.dF", (B, H, S, S), 1.0, 3)).to(dev)
    dT = (1e-4 * weights.det_normal("roofline.dT", (B, 3, S, S), 1.0, 4)).to(dev)
    packed, layer_bias = renderer._derived_buffers()
    packed_t = renderer._packed_transposed()
    run = lambda: nerf_backward_fused(net, renderer.sigmoid_beta.detach(), cam, focal, near, far, u, film, layer_bias, packed,
                                      packed_t, S, n_samples, False, dF, dT)
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    P = B * S * S * n_samples
    fwd = 2.0 * 3 * H + (D - 1) * 2.0 * H * H + 2.0 * (H + 3) * H + 2.0 * H * 4
    bwd = D * 2.0 * H * H + 2.0 * 6 * H
    flop = P * (fwd + bwd)
    a = flop / (ms * 1e-3) / 1e12
    peak = 2500.0 / 3
    return {"kernel": "cips3d_nerf_bwd_fused = nerf_stash_kernel (forward recompute, accumulators stashed) + nerf_bwd_kernel "
                      "(register-resident MFMA backward); timed stand-alone on the step's shape",
            "bound": "mfma", "achieved": a, "peak": peak, "unit": "TFLOP/s", "frac": a / peak,
            "peak_definition": "fp16 dense MFMA peak 2500 TFLOP/s / 3 fp16 products per fp32 product",
            "avg_launch_ms": ms, "flop_per_launch": flop,
            "stash_bytes_per_launch": 2.0 * 4 * P * D * H,
            "note": "stash written once and read once: at this time it moves at %.2f TB/s" % (2.0 * 4 * P * D * H / (ms * 1e-3) / 1e12)}


def sqdiff_pair(a0, b0, c0, a1, b1, c1):
    """loss = c0 sum (a0 - b0)^2 + c1 sum (a1 - b1)^2 as a device scalar (cips3d_sqdiff_pair: the two squared-difference terms
    of the inversion loss, projector_v10.py:1173-1174), deterministic; a1 / b1 may be None."""
    lib = _lib.load()
    n0, n1 = a0.numel(), (a1.numel() if a1 is not None else 0)
    partial = torch.empty(2 * int(lib.cips3d_sqdiff_pair_partials(n0, n1)), device=a0.device)
    loss = torch.empty((), device=a0.device)
    check(lib.cips3d_sqdiff_pair(dev_ptr(a0, "a0"), dev_ptr(b0, "b0"), n0, float(c0), dev_ptr(a1, "a1", True), dev_ptr(b1, "b1", True),
                                 n1, float(c1), partial.data_ptr(), loss.data_ptr(), stream_ptr()), "cips3d_sqdiff_pair")
    return loss


def sqdiff_pair_bwd(a0, b0, c0, a1, b1, c1, gloss):
    """(d loss / d a0, d loss / d a1) of sqdiff_pair for the incoming gradient `gloss` (a device scalar), one launch."""
    lib = _lib.load()
    n0, n1 = a0.numel(), (a1.numel() if a1 is not None else 0)
    d0 = torch.empty_like(a0)
    d1 = torch.empty_like(a1) if a1 is not None else None
    check(lib.cips3d_sqdiff_pair_bwd(dev_ptr(a0, "a0"), dev_ptr(b0, "b0"), n0, float(c0), d0.data_ptr(), dev_ptr(a1, "a1", True),
                                     dev_ptr(b1, "b1", True), n1, float(c1), dev_ptr(d1, "d1", True), dev_ptr(gloss, "gloss"),
                                     stream_ptr()), "cips3d_sqdiff_pair_bwd")
    return d0, d1


# ------------------------------------------------------------------------------- inversion loss terms (csrc/inversion_loss.hip)
def noise_reg_supported(bufs):
    """True when cips3d_noise_reg takes every buffer of the list: fp32 contiguous HIP tensors [B,1,S,S] whose pooled levels all
    have even sides (cips3d_noise_reg_supported)."""
    if len(bufs) == 0:
        return False
    lib = _lib.load()
    return all(b.is_cuda and b.dtype == torch.float32 and b.dim() == 4 and b.shape[1] == 1 and b.shape[2] == b.shape[3]
               and b.is_contiguous() and b.device == bufs[0].device
               and lib.cips3d_noise_reg_supported(b.shape[0], b.shape[2]) == 1 for b in bufs)


def _noise_table(bufs, grads=None):
    tab = (_lib.NoiseBuf * len(bufs))()
    for i, b in enumerate(bufs):
        tab[i].v, tab[i].B, tab[i].S = dev_ptr(b, "noise buffer"), b.shape[0], b.shape[2]
        tab[i].d = grads[i].data_ptr() if grads is not None else None
    return tab


def noise_reg(bufs, weight):
    """weight x the noise regulariser of projector_v10.py:1183-1195 over the whole list `bufs` -> (loss: device scalar,
    workspace: the pyramids and the per-level means noise_reg_bwd reads).  At most four launches per 32 buffers."""
    lib = _lib.load()
    tab = _noise_table(bufs)
    nbytes = int(lib.cips3d_noise_reg_workspace(tab, len(bufs)))
    if nbytes < 0:
        raise RuntimeError("cips3d_noise_reg: unsupported noise buffer shape (hip.noise_reg_supported)")
    ws = torch.empty(nbytes // 4, device=bufs[0].device)
    loss = torch.empty((), device=bufs[0].device)
    check(lib.cips3d_noise_reg(tab, len(bufs), float(weight), ws.data_ptr(), loss.data_ptr(), stream_ptr()), "cips3d_noise_reg")
    return loss, ws


def noise_reg_bwd(bufs, weight, ws, gloss):
    """[gloss x d loss / d v for v in bufs] of noise_reg (same `bufs`, `weight` and its workspace), one launch per 32 buffers."""
    lib = _lib.load()
    grads = [torch.empty_like(b) for b in bufs]
    tab = _noise_table(bufs, grads)
    check(lib.cips3d_noise_reg_bwd(tab, len(bufs), float(weight), dev_ptr(ws, "workspace"), dev_ptr(gloss, "gloss"), stream_ptr()),
          "cips3d_noise_reg_bwd")
    return grads


def mask_blend_factor(x, mask):
    """The integer up-sampling factor of cips3d_mask_blend for image x [B,C,H,W] and mask [B,1,h,w], or 0 when the pair is not
    one the kernel takes (fp32 contiguous HIP tensors, H / h = W / w an integer >= 1)."""
    if not (x.is_cuda and mask.is_cuda and x.dtype == torch.float32 and mask.dtype == torch.float32 and x.dim() == 4
            and mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[0] == x.shape[0] and x.device == mask.device):
        return 0
    H, W, h, w = x.shape[2], x.shape[3], mask.shape[2], mask.shape[3]
    if h < 1 or w < 1 or H < h or H % h or W % w or H // h != W // w:
        return 0
    return H // h


def mask_blend(x, mask, backward=False):
    """x m + x (1 - m) -- or, with `backward`, x m for x = the incoming gradient -- with m the bicubic up-sampling of 1 - mask
    evaluated inside the kernel (cips3d_mask_blend / _bwd: projector_v10.py:1164-1167, :268-273)."""
    lib = _lib.load()
    f = mask_blend_factor(x, mask)
    if f == 0:
        raise RuntimeError(f"cips3d_mask_blend: image {tuple(x.shape)} / mask {tuple(mask.shape)} is not an integer up-sampling")
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    fn = lib.cips3d_mask_blend_bwd if backward else lib.cips3d_mask_blend
    check(fn(dev_ptr(x, "x"), dev_ptr(mask, "mask"), out.data_ptr(), B, Cc, H, W, f, stream_ptr()),
          "cips3d_mask_blend_bwd" if backward else "cips3d_mask_blend")
    return out


# ------------------------------------------------------------------------------- Gaussian-window SSIM loss (csrc/ssim_loss.hip)
SSIM_WIN = 11                   # taps of the window; a side below it has no window


def ssim_loss_tile():
    """(tile_h, tile_w, threads) of cips3d_ssim_loss: the sides of a workgroup's tile of window origins and its thread count."""
    th, tw = C.c_int(0), C.c_int(0)
    threads = _lib.load().cips3d_ssim_loss_tile(C.byref(th), C.byref(tw))
    return th.value, tw.value, threads


def ssim_loss_supported(a, b):
    """True when cips3d_ssim_loss takes the pair: fp32 HIP tensors [B,C,H,W] of equal shape on one device, C in {1, 3}, both
    sides >= 11."""
    return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.is_cuda and b.is_cuda and a.device == b.device
            and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 4 and a.shape == b.shape
            and a.shape[0] >= 1 and a.shape[1] in (1, 3) and a.shape[2] >= SSIM_WIN and a.shape[3] >= SSIM_WIN)


def ssim_loss_workspace_bytes(B, Cc, H, W, need_grad):
    n = int(_lib.load().cips3d_ssim_loss_workspace_bytes(B, Cc, H, W, int(bool(need_grad))))
    if n < 0:
        raise RuntimeError(f"cips3d_ssim_loss_workspace_bytes({B}, {Cc}, {H}, {W}) failed ({n})")
    return n


def ssim_loss(a, b, weight=1.0, data_range=2.0, need_grad=False, return_map=False):
    """weight x mean_i (1 - ssim_i) of the Gaussian-window SSIM of a against b (cips3d_ssim_loss: two launches, nothing read back)
    -> (loss: fp32 device scalar, ssim: float64 [B] on the device, workspace, map or None).  `need_grad`: the workspace also
    holds the three derivative maps ssim_loss_bwd reads.  `return_map`: S per window, [B,C,H-10,W-10]."""
    lib = _lib.load()
    if not ssim_loss_supported(a, b):
        raise RuntimeError("cips3d_ssim_loss: fp32 HIP tensors [B,C,H,W] of equal shape, C in {1, 3}, sides >= 11 (hip.ssim_loss_supported)")
    B, Cc, H, W = a.shape
    ws = torch.empty((ssim_loss_workspace_bytes(B, Cc, H, W, need_grad) + 3) // 4, device=a.device)
    ssim = torch.empty(B, dtype=torch.float64, device=a.device)
    loss = torch.empty((), device=a.device)
    smap = torch.empty(B, Cc, H - SSIM_WIN + 1, W - SSIM_WIN + 1, device=a.device) if return_map else None
    check(lib.cips3d_ssim_loss(dev_ptr(a, "a"), dev_ptr(b, "b"), B, Cc, H, W, float(weight), float(data_range), ws.data_ptr(),
                               int(bool(need_grad)), dev_ptr(smap, "map", True), ssim.data_ptr(), loss.data_ptr(), stream_ptr()),
          "cips3d_ssim_loss")
    return loss, ssim, ws, smap


def ssim_loss_bwd(a, b, weight, ws, gloss):
    """gloss x d loss / d a of ssim_loss(a, b, weight, need_grad=True) with its workspace `ws`; gloss a device scalar.  One launch."""
    lib = _lib.load()
    B, Cc, H, W = a.shape
    da = torch.empty_like(a)
    check(lib.cips3d_ssim_loss_bwd(dev_ptr(a, "a"), dev_ptr(b, "b"), B, Cc, H, W, float(weight), dev_ptr(ws, "workspace"),
                                   dev_ptr(gloss, "gloss"), da.data_ptr(), stream_ptr()), "cips3d_ssim_loss_bwd")
    return da


# ---------------------------------------------------------------------------------------------- geometry export (csrc/mesh.hip)
def align_volume(volume, near=0.88, far=1.12, out=None):
    """cips3d_align_volume: volume [B,h,w,d] fp32 -> the frustum-aligned volume of the same shape."""
    lib = _lib.load()
    if volume.dim() != 4:
        raise RuntimeError("align_volume: volume must be [B, h, w, d]")
    B, h, w, d = volume.shape
    if out is None:
        out = torch.empty_like(volume)
    check(lib.cips3d_align_volume(dev_ptr(volume, "volume"), dev_ptr(out, "out"), B, h, w, d, float(near), float(far),
                                  stream_ptr()), "cips3d_align_volume")
    return out


def marching_cubes_count(vol, level=0.0):
    """cips3d_marching_cubes_count on vol [h,w,d] fp32 -> (workspace, totals: device int32 [2] = V, F), enqueued only."""
    lib = _lib.load()
    if vol.dim() != 3:
        raise RuntimeError("marching_cubes: vol must be [h, w, d]")
    h, w, d = vol.shape
    ws_bytes = lib.cips3d_marching_cubes_workspace_bytes(h, w, d)
    if ws_bytes < 0:
        check(int(ws_bytes), "cips3d_marching_cubes_workspace_bytes")
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=vol.device)
    totals = torch.empty(2, dtype=torch.int32, device=vol.device)
    check(lib.cips3d_marching_cubes_count(dev_ptr(vol, "vol"), h, w, d, float(level), ws.data_ptr(), totals.data_ptr(),
                                          stream_ptr()), "cips3d_marching_cubes_count")
    return ws, totals


def marching_cubes_emit(vol, level, ws, n_verts, n_faces, affine=None):
    """cips3d_marching_cubes_emit after marching_cubes_count (same vol, level, workspace) -> (verts [V,3] fp32,
    faces [F,3] int32).  `affine`: ((sx, ox), (sy, oy), (sz, oz)) per axis on index-space positions (None: index space)."""
    lib = _lib.load()
    h, w, d = vol.shape
    verts = torch.empty(n_verts, 3, dtype=torch.float32, device=vol.device)
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=vol.device)
    aff = None if affine is None else (C.c_float * 6)(*[float(v) for pair in affine for v in pair])
    check(lib.cips3d_marching_cubes_emit(dev_ptr(vol, "vol"), h, w, d, float(level), aff, ws.data_ptr(),
                                         verts.data_ptr() if n_verts else None, faces.data_ptr() if n_faces else None,
                                         n_verts, n_faces, stream_ptr()), "cips3d_marching_cubes_emit")
    return verts, faces


def marching_cubes_normals(vol, level, ws, n_verts, affine=None):
    """cips3d_marching_cubes_normals after marching_cubes_count (same vol, level, workspace) -> unit normals [V,3] fp32 in the
    emit call's vertex order: the volume's lattice gradient interpolated along each vertex's edge, in the affine's frame."""
    lib = _lib.load()
    h, w, d = vol.shape
    normals = torch.empty(n_verts, 3, dtype=torch.float32, device=vol.device)
    aff = None if affine is None else (C.c_float * 6)(*[float(v) for pair in affine for v in pair])
    check(lib.cips3d_marching_cubes_normals(dev_ptr(vol, "vol"), h, w, d, float(level), aff, ws.data_ptr(),
                                            normals.data_ptr() if n_verts else None, n_verts, stream_ptr()),
          "cips3d_marching_cubes_normals")
    return normals


def marching_cubes(vol, level=0.0, affine=None, normals=False):
    """Marching cubes on one volume [h,w,d] fp32 -> (verts [V,3] fp32, faces [F,3] int64) on its device (contract:
    include/cips3d_hip.h).  Reading the two totals is the one host synchronisation; the outputs are allocated from them.
    normals=True: a third value, the unit vertex normals [V,3] fp32 (marching_cubes_normals)."""
    ws, totals = marching_cubes_count(vol, level)
    n_v, n_f = (int(v) for v in totals.cpu())
    verts, faces = marching_cubes_emit(vol, level, ws, n_v, n_f, affine)
    if normals:
        return verts, faces.long(), marching_cubes_normals(vol, level, ws, n_v, affine)
    return verts, faces.long()


def mc_case_table():
    """The library's case table (host only): (tri_count [256] int32, tri_edges [256, width, 3] int32, -1 padded)."""
    import numpy as np
    lib = _lib.load()
    width = lib.cips3d_mc_table_width()
    cnt = np.zeros(256, np.int32)
    edges = np.zeros((256, width, 3), np.int32)
    check(lib.cips3d_mc_case_table(cnt.ctypes.data, edges.ctypes.data), "cips3d_mc_case_table")
    return cnt, edges


# ---------------------------------------------------------------------------------------------- mesh rasteriser (csrc/mesh_raster.hip)
def mesh_raster_workspace(n_verts, n_faces, n_views, image_size, device):
    """(workspace, keys [n,S,S] int64 holding the uint64 keys) for mesh_rasterize / mesh_resolve at these sizes."""
    lib = _lib.load()
    nbytes = lib.cips3d_mesh_raster_workspace_bytes(int(n_verts), int(n_faces), int(n_views), int(image_size))
    if nbytes < 0:
        check(int(nbytes), "cips3d_mesh_raster_workspace_bytes")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    keys = torch.empty(int(n_views), int(image_size), int(image_size), dtype=torch.int64, device=device)
    return ws, keys


def mesh_rasterize(verts, faces, cams, image_size, ws=None, keys=None):
    """cips3d_mesh_rasterize: verts [V,3] fp32, faces [F,3] int32, cams [n,5] fp32 (azim, elev, fov_deg, dist, znear) ->
    (workspace, keys), enqueued only; the key buffer is cleared by the call.  `ws` / `keys`: buffers of
    mesh_raster_workspace for the same sizes, reused."""
    lib = _lib.load()
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("mesh_rasterize: verts must be [V, 3], faces [F, 3]")
    if cams.dim() != 2 or cams.shape[1] != 5:
        raise RuntimeError("mesh_rasterize: cams must be [n, 5] = (azim, elev, fov_deg, dist, znear)")
    V, F, n, S = verts.shape[0], faces.shape[0], cams.shape[0], int(image_size)
    if ws is None or keys is None:
        ws, keys = mesh_raster_workspace(V, F, n, S, verts.device)
    elif keys.shape != (n, S, S) or keys.dtype != torch.int64 or \
            ws.numel() < lib.cips3d_mesh_raster_workspace_bytes(V, F, n, S):
        raise RuntimeError("mesh_rasterize: workspace / keys do not fit these sizes")
    check(lib.cips3d_mesh_rasterize(dev_ptr(verts, "verts") if V else None,
                                    V, dev_ptr(faces, "faces", dtype=torch.int32) if F else None, F, dev_ptr(cams, "cams"), n, S,
                                    dev_ptr(ws, "ws", dtype=torch.uint8), dev_ptr(keys, "keys", dtype=torch.int64), stream_ptr()),
          "cips3d_mesh_rasterize")
    return ws, keys


def mesh_resolve(verts, faces, ws, keys, want=("face", "zbuf", "bary"), attr=None, base=None, fill=0.0, normals=None, light=None,
                 ka=None, kd=None, ks=None, shininess=None, out=None):
    """cips3d_mesh_resolve after mesh_rasterize (same verts, faces, workspace, keys) -> dict with the entries named in `want`
    (and every entry `out` holds a tensor for): face [n,S,S] int32, zbuf [n,S,S], bary [n,S,S,3], attr [n,C,S,S] (needs attr
    [V,C]; empty pixels take `base` [n,C,S,S] when given, else `fill`), shade [n,S,S], shade_u8 [n,3,S,S] uint8 (need
    normals [V,3] and light [n,3]).  ka / kd / ks / shininess default to PHONG_DEFAULTS."""
    lib = _lib.load()
    n, S = keys.shape[0], keys.shape[1]
    V, F = verts.shape[0], faces.shape[0]
    out = dict(out or {})
    names = set(want) | set(out)
    unknown = names - {"face", "zbuf", "bary", "attr", "shade", "shade_u8"}
    if unknown:
        raise RuntimeError(f"mesh_resolve: unknown outputs {sorted(unknown)}")
    if "attr" in names and attr is None:
        raise RuntimeError("mesh_resolve: the attr output needs attr")
    if names & {"shade", "shade_u8"} and (normals is None or light is None):
        raise RuntimeError("mesh_resolve: the shade outputs need normals and light")
    n_attr = 0
    if "attr" in names:
        if attr.dim() != 2 or attr.shape[0] != V:
            raise RuntimeError("mesh_resolve: attr must be [V, C]")
        n_attr = attr.shape[1]
    shapes = {"face": ((n, S, S), torch.int32), "zbuf": ((n, S, S), torch.float32), "bary": ((n, S, S, 3), torch.float32),
              "attr": ((n, n_attr, S, S), torch.float32), "shade": ((n, S, S), torch.float32),
              "shade_u8": ((n, 3, S, S), torch.uint8)}
    for name in names:
        shape, dt = shapes[name]
        if out.get(name) is None:
            out[name] = torch.empty(shape, dtype=dt, device=verts.device)
        elif tuple(out[name].shape) != shape:
            raise RuntimeError(f"mesh_resolve: {name} must be {shape}")
    if base is not None and tuple(base.shape) != shapes["attr"][0]:
        raise RuntimeError(f"mesh_resolve: base must be {shapes['attr'][0]}")
    if normals is not None and tuple(normals.shape) != (V, 3):
        raise RuntimeError("mesh_resolve: normals must be [V, 3]")
    if light is not None and tuple(light.shape) != (n, 3):
        raise RuntimeError("mesh_resolve: light must be [n, 3]")
    ph = dict(PHONG_DEFAULTS)
    ph.update({k: float(v) for k, v in dict(ka=ka, kd=kd, ks=ks, shininess=shininess).items() if v is not None})

    def ptr(t, name, dtype=torch.float32):
        return None if t is None or t.numel() == 0 else dev_ptr(t, name, dtype=dtype)
    p = _lib.MeshResolveParams(
        verts=ptr(verts, "verts"), faces=ptr(faces, "faces", torch.int32), workspace=dev_ptr(ws, "ws", dtype=torch.uint8),
        keys=dev_ptr(keys, "keys", dtype=torch.int64), face=ptr(out.get("face"), "face", torch.int32),
        zbuf=ptr(out.get("zbuf"), "zbuf"), bary=ptr(out.get("bary"), "bary"), attr=ptr(attr, "attr") if "attr" in names else None,
        base=ptr(base, "base"), attr_out=ptr(out.get("attr"), "attr_out"), normals=ptr(normals, "normals"),
        light=ptr(light, "light"), shade=ptr(out.get("shade"), "shade"), shade_u8=ptr(out.get("shade_u8"), "shade_u8", torch.uint8),
        V=V, F=F, n_views=n, S=S, n_attr=n_attr, fill=float(fill), **ph)
    check(lib.cips3d_mesh_resolve(C.byref(p), stream_ptr()), "cips3d_mesh_resolve")
    return out


# ---------------------------------------------------------------------------------------------- mesh colours (csrc/mesh_color.hip)
def mesh_vertex_colors(verts, normals, images, ws, keys, S, power=2, depth_tol=0.0, fill=0.0, want=("colors", "weight", "seen"),
                       out=None):
    """cips3d_mesh_vertex_colors after mesh_rasterize (same verts, workspace, keys, S): verts / normals [V,3] fp32, images
    [n,3,R,R] fp32, one per rasterised view -> dict with the entries named in `want` (and every entry `out` holds a tensor
    for): colors [V,3] fp32, weight [V] fp32, seen [V] int32.  Enqueued only."""
    lib = _lib.load()
    V, n, S = verts.shape[0], keys.shape[0], int(S)
    if verts.dim() != 2 or verts.shape[1] != 3 or tuple(normals.shape) != (V, 3):
        raise RuntimeError("mesh_vertex_colors: verts and normals must be [V, 3]")
    if images.dim() != 4 or images.shape[0] != n or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
        raise RuntimeError(f"mesh_vertex_colors: images must be [{n}, 3, R, R], one square picture per rasterised view")
    if tuple(keys.shape) != (n, S, S) or ws.numel() < lib.cips3d_mesh_raster_workspace_bytes(V, 0, n, S):
        raise RuntimeError("mesh_vertex_colors: workspace / keys do not fit these sizes")
    out = dict(out or {})
    names = set(want) | set(out)
    shapes = {"colors": ((V, 3), torch.float32), "weight": ((V,), torch.float32), "seen": ((V,), torch.int32)}
    if not names or names - set(shapes):
        raise RuntimeError(f"mesh_vertex_colors: outputs must be among {sorted(shapes)}, at least one")
    for name in names:
        shape, dt = shapes[name]
        if out.get(name) is None:
            out[name] = torch.empty(shape, dtype=dt, device=verts.device)
        elif tuple(out[name].shape) != shape:
            raise RuntimeError(f"mesh_vertex_colors: {name} must be {shape}")

    def ptr(t, name, dtype=torch.float32):
        return None if t is None or t.numel() == 0 else dev_ptr(t, name, dtype=dtype)
    p = _lib.MeshColorParams(
        verts=ptr(verts, "verts"), normals=ptr(normals, "normals"), images=ptr(images, "images"),
        workspace=dev_ptr(ws, "ws", dtype=torch.uint8), keys=dev_ptr(keys, "keys", dtype=torch.int64),
        colors=ptr(out.get("colors"), "colors"), weight=ptr(out.get("weight"), "weight"), seen=ptr(out.get("seen"), "seen", torch.int32),
        V=V, n_views=n, S=S, R=int(images.shape[2]), power=int(power), depth_tol=float(depth_tol), fill=float(fill))
    if V:
        check(lib.cips3d_mesh_vertex_colors(C.byref(p), stream_ptr()), "cips3d_mesh_vertex_colors")
    return out


def mesh_albedo_frame(face, shade, attr, out=None):
    """cips3d_mesh_albedo_frame: mesh_resolve's face [n,S,S] int32, shade [n,S,S] and attr [n,3,S,S] (colours in [-1, 1]) ->
    uint8 [n,3,S,S] = shade x (attr + 1) / 2, white where empty."""
    n, S = face.shape[0], face.shape[1]
    if tuple(face.shape) != (n, S, S) or tuple(shade.shape) != (n, S, S) or tuple(attr.shape) != (n, 3, S, S):
        raise RuntimeError("mesh_albedo_frame: face and shade must be [n, S, S], attr [n, 3, S, S]")
    if out is None:
        out = torch.empty(n, 3, S, S, dtype=torch.uint8, device=face.device)
    elif tuple(out.shape) != (n, 3, S, S):
        raise RuntimeError(f"mesh_albedo_frame: out must be {(n, 3, S, S)}")
    if n:
        check(_lib.load().cips3d_mesh_albedo_frame(dev_ptr(face, "face", dtype=torch.int32), dev_ptr(shade, "shade"),
                                                   dev_ptr(attr, "attr"), dev_ptr(out, "out", dtype=torch.uint8), n, S, stream_ptr()),
              "cips3d_mesh_albedo_frame")
    return out


# ---------------------------------------------------------------------------------------------- mesh texture (csrc/mesh_texture.hip)
def mesh_atlas_layout(n_faces, texels=8, cols=None):
    """cips3d_mesh_atlas_layout (host only): (cols, rows, width, height) of the atlas of n_faces faces at `texels` texels per
    cell side; cols=None: the default."""
    out = [C.c_int32(0) for _ in range(4)]
    if cols is not None and int(cols) < 1:
        raise RuntimeError("mesh_atlas_layout: cols must be at least 1")
    check(_lib.load().cips3d_mesh_atlas_layout(int(n_faces), int(texels), 0 if cols is None else int(cols), *(C.byref(o) for o in out)),
          "cips3d_mesh_atlas_layout")
    return tuple(o.value for o in out)


def mesh_atlas_uv(n_faces, texels, cols):
    """cips3d_mesh_atlas_uv (host only): numpy [F,3,2] fp32, the faces' corner UVs in continuous texel coordinates."""
    import numpy as np
    uv = np.zeros((int(n_faces), 3, 2), np.float32)
    check(_lib.load().cips3d_mesh_atlas_uv(int(n_faces), int(texels), int(cols), uv.ctypes.data if n_faces else None),
          "cips3d_mesh_atlas_uv")
    return uv


def mesh_atlas_texels(n_faces, texels, cols, rows):
    """cips3d_mesh_atlas_texels (host only): numpy (face [Ht,Wt] int32, -1 where unowned; bary [Ht,Wt,3] fp32; gutter [Ht,Wt]
    bool) -- what the bake kernel decides per texel."""
    import numpy as np
    T, cols, rows = int(texels), int(cols), int(rows)
    shape = (max(rows, 0) * T, max(cols, 0) * (T + 1))
    face, bary, gutter = np.zeros(shape, np.int32), np.zeros(shape + (3,), np.float32), np.zeros(shape, np.uint8)
    check(_lib.load().cips3d_mesh_atlas_texels(int(n_faces), T, cols, rows, face.ctypes.data, bary.ctypes.data, gutter.ctypes.data),
          "cips3d_mesh_atlas_texels")
    return face, bary, gutter.astype(bool)


def mesh_fill_colors(colors, weight, faces, iters=64, out=None, ws=None):
    """cips3d_mesh_fill_colors: colors [V,3] fp32, weight [V] fp32, faces [F,3] int32 -> {"colors": [V,3] fp32, "filled": [V]
    int32 (0: seen, r: filled in ring r, -1: never)}.  `out`: tensors to write into; `ws`: a uint8 workspace to reuse.
    Enqueued only."""
    lib = _lib.load()
    V, F = colors.shape[0], faces.shape[0]
    if tuple(colors.shape) != (V, 3) or tuple(weight.shape) != (V,) or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("mesh_fill_colors: colors must be [V, 3], weight [V], faces [F, 3]")
    out = dict(out or {})
    if set(out) - {"colors", "filled"}:
        raise RuntimeError("mesh_fill_colors: outputs are colors and filled")
    for name, shape, dt in (("colors", (V, 3), torch.float32), ("filled", (V,), torch.int32)):
        if out.get(name) is None:
            out[name] = torch.empty(shape, dtype=dt, device=colors.device)
        elif tuple(out[name].shape) != shape:
            raise RuntimeError(f"mesh_fill_colors: {name} must be {shape}")
    nbytes = lib.cips3d_mesh_fill_workspace_bytes(V)
    if nbytes < 0:
        check(int(nbytes), "cips3d_mesh_fill_workspace_bytes")
    if ws is None:
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=colors.device)
    elif ws.numel() < nbytes or ws.data_ptr() % 8:
        raise RuntimeError("mesh_fill_colors: the workspace is too small or not 8-byte aligned (it holds 64-bit sums)")
    if V == 0 or F == 0:                  # the library launches nothing: no ring can reach anything
        if int(iters) < 0 or int(iters) > 4096:
            raise RuntimeError("mesh_fill_colors: iters must lie in 0..4096")
        out["colors"].copy_(colors)
        out["filled"].copy_(torch.where(weight > 0, 0, -1))
        return out
    check(lib.cips3d_mesh_fill_colors(dev_ptr(colors, "colors"), dev_ptr(weight, "weight"), dev_ptr(faces, "faces", dtype=torch.int32),
                                      V, F, int(iters), dev_ptr(out["colors"], "colors_out"),
                                      dev_ptr(out["filled"], "filled", dtype=torch.int32), dev_ptr(ws, "ws", dtype=torch.uint8),
                                      stream_ptr()), "cips3d_mesh_fill_colors")
    return out


def mesh_texture_bake(verts, faces, normals, images, ws, keys, S, T, cols, rows, power=2, depth_tol=0.0, fill=0.0,
                      vertex_colors=None, filled=None, want=("texture", "weight", "seen"), out=None):
    """cips3d_mesh_texture_bake after mesh_rasterize (same verts, faces, workspace, keys, S) into the atlas (T, cols, rows) of
    mesh_atlas_layout -> dict with the entries named in `want` (and every entry `out` holds a tensor for): texture [3,Ht,Wt]
    fp32, weight [Ht,Wt] fp32, seen [Ht,Wt] int32.  vertex_colors [V,3] / filled [V] int32 (mesh_fill_colors), both or neither:
    the colour of the texels no view sees.  Enqueued only."""
    lib = _lib.load()
    V, F, n, S = verts.shape[0], faces.shape[0], keys.shape[0], int(S)
    T, cols, rows = int(T), int(cols), int(rows)
    if verts.dim() != 2 or verts.shape[1] != 3 or tuple(normals.shape) != (V, 3) or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("mesh_texture_bake: verts and normals must be [V, 3], faces [F, 3]")
    if images.dim() != 4 or images.shape[0] != n or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
        raise RuntimeError(f"mesh_texture_bake: images must be [{n}, 3, R, R], one square picture per rasterised view")
    if tuple(keys.shape) != (n, S, S) or ws.numel() < lib.cips3d_mesh_raster_workspace_bytes(V, F, n, S):
        raise RuntimeError("mesh_texture_bake: workspace / keys do not fit these sizes")
    if (vertex_colors is None) != (filled is None):
        raise RuntimeError("mesh_texture_bake: give vertex_colors and filled together")
    if vertex_colors is not None and (tuple(vertex_colors.shape) != (V, 3) or tuple(filled.shape) != (V,)):
        raise RuntimeError("mesh_texture_bake: vertex_colors must be [V, 3], filled [V]")
    if T < 3 or T > 64 or cols < 1 or rows < 0 or cols * rows < (F + 1) // 2:
        raise RuntimeError(f"mesh_texture_bake: an atlas of {cols} x {rows} cells of {T} texels does not hold {F} faces")
    Ht, Wt = rows * T, cols * (T + 1)
    out = dict(out or {})
    names = set(want) | set(out)
    shapes = {"texture": ((3, Ht, Wt), torch.float32), "weight": ((Ht, Wt), torch.float32), "seen": ((Ht, Wt), torch.int32)}
    if not names or names - set(shapes):
        raise RuntimeError(f"mesh_texture_bake: outputs must be among {sorted(shapes)}, at least one")
    for name in names:
        shape, dt = shapes[name]
        if out.get(name) is None:
            out[name] = torch.empty(shape, dtype=dt, device=verts.device)
        elif tuple(out[name].shape) != shape:
            raise RuntimeError(f"mesh_texture_bake: {name} must be {shape}")

    def ptr(t, name, dtype=torch.float32):
        return None if t is None or t.numel() == 0 else dev_ptr(t, name, dtype=dtype)
    p = _lib.MeshTextureParams(
        verts=ptr(verts, "verts"), faces=ptr(faces, "faces", torch.int32), normals=ptr(normals, "normals"), images=ptr(images, "images"),
        workspace=dev_ptr(ws, "ws", dtype=torch.uint8), keys=dev_ptr(keys, "keys", dtype=torch.int64),
        vertex_colors=ptr(vertex_colors, "vertex_colors"), filled=ptr(filled, "filled", torch.int32),
        texture=ptr(out.get("texture"), "texture"), weight=ptr(out.get("weight"), "weight"), seen=ptr(out.get("seen"), "seen", torch.int32),
        V=V, F=F, n_views=n, S=S, R=int(images.shape[2]), power=int(power), T=T, cols=cols, rows=rows, depth_tol=float(depth_tol),
        fill=float(fill))
    if V and F:
        check(lib.cips3d_mesh_texture_bake(C.byref(p), stream_ptr()), "cips3d_mesh_texture_bake")
    return out


def mesh_textured_frame(face, bary, shade, texture, n_faces, T, cols, rows, out=None):
    """cips3d_mesh_textured_frame: mesh_resolve's face [n,S,S] int32, bary [n,S,S,3] and shade [n,S,S], texture [3,Ht,Wt] of the
    atlas (T, cols, rows) for n_faces faces -> uint8 [n,3,S,S] = shade x (texel + 1) / 2, white where empty.  Enqueued only."""
    n, S = face.shape[0], face.shape[1]
    T, cols, rows, F = int(T), int(cols), int(rows), int(n_faces)
    if tuple(face.shape) != (n, S, S) or tuple(shade.shape) != (n, S, S) or tuple(bary.shape) != (n, S, S, 3):
        raise RuntimeError("mesh_textured_frame: face and shade must be [n, S, S], bary [n, S, S, 3]")
    if tuple(texture.shape) != (3, rows * T, cols * (T + 1)):
        raise RuntimeError(f"mesh_textured_frame: texture must be {(3, rows * T, cols * (T + 1))}")
    if out is None:
        out = torch.empty(n, 3, S, S, dtype=torch.uint8, device=face.device)
    elif tuple(out.shape) != (n, 3, S, S):
        raise RuntimeError(f"mesh_textured_frame: out must be {(n, 3, S, S)}")
    if n and F == 0:
        out.fill_(255)                        # no face: every pixel is empty (the library launches nothing)
    elif n:
        check(_lib.load().cips3d_mesh_textured_frame(dev_ptr(face, "face", dtype=torch.int32), dev_ptr(bary, "bary"),
                                                     dev_ptr(shade, "shade"), dev_ptr(texture, "texture"),
                                                     dev_ptr(out, "out", dtype=torch.uint8), n, S, F, T, cols, rows, stream_ptr()),
              "cips3d_mesh_textured_frame")
    return out


# ---------------------------------------------------------------------------------------------- VGG16 conv loss (csrc/vgg.hip)
def vgg_supported(B, H, W):
    """cips3d_vgg_supported as a bool: B >= 1, H and W multiples of 16 (decided on the host; perceptual.VGG16ConvLoss)."""
    return _lib.load().cips3d_vgg_supported(int(B), int(H), int(W)) == 0


def vgg_check_supported(B, H, W):
    code = _lib.load().cips3d_vgg_supported(int(B), int(H), int(W))
    if code != 0:
        raise RuntimeError(f"VGG16 conv loss: B = {B}, H = {H}, W = {W} is outside the size contract (B >= 1, H and W multiples "
                           f"of 16): {_lib.load().cips3d_strerror(code).decode()}")
