"""Views in flight on the GPU: pipeline.ViewPipeline's lanes against the one-stream forward, bit for bit.

The reference project renders one view per call on one stream, so the reference of every check here is this package's own one-stream
forward (pinned to the oracle and the goldens by test_gpu_parity.py / test_gpu_reference_fixtures.py), and every comparison is
`torch.equal`: bit identity is the documented contract (README), there is no tolerance to choose.

Orderings are made observable with `delay()`: a bounded busy kernel on one stream that holds back everything enqueued behind it for
~20 ms, far longer than any forward of these sizes takes.  A missing wait then reads memory that has not been written yet -- every
time, not by luck."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
S, N = 64, 6                      # NeRF resolution and samples per ray of the planned generator's cases
KEYS = ("rgb", "thumb_rgb", "xyz", "mask", "depth", "sdf")


def _pkg():
    import cips_3dplusplus_amd as pkg
    from cips_3dplusplus_amd import configs
    return pkg, configs


# ------------------------------------------------------------------------------------------------------------------ helpers
_SPIN = {}


def delay(ms=20.0):
    """~ms of device time on the CURRENT stream (pipeline._overtakes' spin: torch.cuda._sleep, else a bounded chain of passes over
    a 16 MB tensor), calibrated once.  Bounded: no hang, no fault."""
    if not _SPIN:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        try:
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            a.record(); torch.cuda._sleep(2_000_000); b.record()
            torch.cuda.synchronize()
            _SPIN["cycles_per_ms"] = 2_000_000 / max(a.elapsed_time(b), 1e-3)
        except Exception:                             # noqa: BLE001  (no spin kernel in this build)
            x = _SPIN["x"] = torch.zeros(1 << 22, device=DEV)
            x.add_(1.0)
            torch.cuda.synchronize()
            a.record()
            for _ in range(100):
                x.add_(1.0)
            b.record()
            torch.cuda.synchronize()
            _SPIN["passes_per_ms"] = 100 / max(a.elapsed_time(b), 1e-3)
    if "cycles_per_ms" in _SPIN:
        torch.cuda._sleep(int(min(ms * _SPIN["cycles_per_ms"], 2e9)))
    else:
        for _ in range(int(min(ms * _SPIN["passes_per_ms"], 20000))):
            _SPIN["x"].add_(1.0)


def G256(seed=3):
    """The smallest generator whose forward is planned; at B = 1 its 512 -> 512 layers at 64^2 meet the half-chip condition
    (B * (Cout / 64) * ceil(HW / 128) = 256), so the views-in-flight hint changes the tiles it runs on."""
    pkg, configs = _pkg()
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=seed)
    return G


def noise_for(G, img_size, seed=77):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(b.shape, device=DEV, generator=g) for b in G.create_noise_bufs(img_size, DEV)]


def views(K, B, seed=5, z_dim=256, img_size=S, n_samples=N, noise_bufs=None, **extra):
    """K distinct keyword sets of a forward: distinct latents, camera locations and per-ray jitter, from seeded generators."""
    from cips_3dplusplus_amd.camera import Camera
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(K):
        zs = [torch.randn(B, z_dim, device=DEV, generator=g), torch.randn(B, z_dim, device=DEV, generator=g)]
        locs = torch.randn(B, 2, device=DEV, generator=g) * 0.3
        cam, foc, near, far = Camera.generate_camera_params(img_size, DEV, locations=locs)[:4]
        u = torch.rand(B, img_size, img_size, 1, device=DEV, generator=g)
        out.append(dict(zs=zs, cam_poses=cam, focals=foc, img_size=img_size, near=near, far=far, perturb_u=u, noise_bufs=noise_bufs,
                        nerf_cfg=dict(N_samples=n_samples, perturb=True, static_viewdirs=False), return_sdf=True, return_xyz=True,
                        **extra))
    return out


def serial(G, vs):
    """Every view on the current stream, no pipeline; the results are cloned."""
    with torch.no_grad():
        return [{k: v.clone() for k, v in G(**kw).items() if torch.is_tensor(v)} for kw in vs]


def same(a, b, what=""):
    for k in KEYS:
        assert torch.is_tensor(a[k]) and torch.is_tensor(b[k]), (what, k)
        assert torch.equal(a[k], b[k]), (what, k)


def piped(pipe, vs, lanes=None):
    """The views through the pipeline (alternating lanes, or lanes[i]), drained and synchronised."""
    with torch.no_grad():
        outs = [pipe.submit(lane=None if lanes is None else lanes[i], **kw) for i, kw in enumerate(vs)]
    pipe.drain()
    torch.cuda.synchronize()
    return outs


def lane_of(G, stream):
    return G.__dict__["_stream_lanes"][stream.cuda_stream]


@pytest.fixture(scope="module")
def gen():
    """One planned generator, its noise buffers and the serial reference of each (B, precision) case, computed once."""
    G = G256(3)
    assert G._forward_plan(1, S, N, False) is not None
    nb = noise_for(G, S)
    refs = {}

    def case(B, precision, K):
        key = (B, precision)
        if key not in refs:
            vs = views(K, B, seed=5 + B, noise_bufs=nb)
            G.set_precision(precision)
            try:
                refs[key] = (vs, serial(G, vs))
            finally:
                G.set_precision("fp32")
        vs, ref = refs[key]
        assert len(vs) >= K
        return vs[:K], ref[:K]

    return G, nb, case


# ------------------------------------------------------------------------------------------------- 1. lanes equal one stream
@pytest.mark.parametrize("B,precision,K,lanes", [(1, "fp32", 16, 2), (2, "fp32", 16, 2), (1, "bf16_storage", 6, 2),
                                                 (1, "fp32_exact", 6, 2), (1, "fp32", 16, 3)])
def test_lanes_equal_one_stream(gen, B, precision, K, lanes):
    """K alternating submits on `lanes` streams == the same calls one after the other on one stream, every output, twice.
    (1, fp32): the views-in-flight hint selects the half-chip 128 x 128 chain tiles; (2, fp32): the hint is given but the 512
    tiles stay 64 x 128; the other precisions take other kernels through the same plans."""
    from cips_3dplusplus_amd.pipeline import ViewPipeline
    G, _, case = gen
    vs, ref = case(B, precision, K)
    G.set_precision(precision)
    try:
        pipe = ViewPipeline(G, lanes=lanes)
        assert pipe.lanes == lanes and len({s.cuda_stream for s in pipe.streams}) == lanes
        first = piped(pipe, vs)
        second = piped(pipe, vs)
    finally:
        G.set_precision("fp32")
    for i in range(K):
        same(first[i], ref[i], ("first", i))
        same(second[i], ref[i], ("second", i))
        same(first[i], second[i], ("passes", i))
    plan = G.__dict__["_lane_plans"][lane_of(G, pipe.streams[1])][(B, S, N, False)]
    assert plan is not None and plan.lane == lane_of(G, pipe.streams[1]) != 0
    assert G._views_in_flight == 1


# ------------------------------------------------------------------------------------------ 2. the hint alone changes no bit
def test_views_in_flight_hint_changes_no_bit(gen):
    """The whole-forward form of test_half_chip_tiles_give_the_same_bits: one view, one stream, hint 2 against hint 1."""
    G, _, case = gen
    vs, ref = case(1, "fp32", 16)
    try:
        G._views_in_flight = 2
        hinted = serial(G, vs[:2])
        G._views_in_flight = 1
        plain = serial(G, vs[:2])
    finally:
        G._views_in_flight = 1
    torch.cuda.synchronize()
    for i in range(2):
        same(hinted[i], plain[i], ("hint", i))
        same(plain[i], ref[i], ("reference", i))


# ---------------------------------------------------------------------------------------------------- 3. fresh noise and jitter
def test_fresh_noise_and_jitter_follow_the_call_order(gen):
    """noise_bufs=None and perturb=True without perturb_u: the draws belong to the call, in call order, whatever lane runs it."""
    from cips_3dplusplus_amd.pipeline import ViewPipeline
    G, _, _ = gen
    vs = [{**kw, "noise_bufs": None, "perturb_u": None} for kw in views(6, 1, seed=21)]
    torch.manual_seed(5)
    ref = serial(G, vs)
    torch.manual_seed(5)
    outs = piped(ViewPipeline(G, lanes=2), vs)
    for i in range(6):
        same(outs[i], ref[i], i)
    same_inputs = [{**vs[0]}, {**vs[0]}]
    torch.manual_seed(5)
    a, b = serial(G, same_inputs)
    assert not torch.equal(a["rgb"], b["rgb"]) and not torch.equal(a["sdf"], b["sdf"])       # the draw did advance
    assert not torch.equal(ref[0]["rgb"], ref[1]["rgb"])


# ------------------------------------------------------------------------------------------- 4. wait_inputs / drain / wait_lane
def test_the_lane_waits_for_the_callers_inputs(gen):
    """(a) the inputs are made on the caller's stream BEHIND a delay and submitted at once: the lane must wait for them."""
    from cips_3dplusplus_amd.pipeline import ViewPipeline
    G, nb, _ = gen
    pipe = ViewPipeline(G, lanes=2)
    delay()
    vs = views(2, 1, seed=31, noise_bufs=nb)           # (enqueued behind the delay: not written yet when submit returns)
    with torch.no_grad():
        outs = [pipe.submit(**kw) for kw in vs]
    pipe.drain()
    torch.cuda.synchronize()
    ref = serial(G, vs)
    for i in range(2):
        same(outs[i], ref[i], i)


@pytest.mark.parametrize("how", ["drain", "wait_lane"])
def test_the_caller_waits_for_the_lane(gen, how):
    """(b), (c): the forward sits behind a delay on its lane; after drain() / wait_lane(last_lane) a clone on the caller's stream,
    with no host synchronisation in between, must see the finished image."""
    from cips_3dplusplus_amd.pipeline import ViewPipeline
    G, nb, _ = gen
    vs = views(1, 1, seed=32, noise_bufs=nb)
    ref = serial(G, vs)
    torch.cuda.synchronize()
    pipe = ViewPipeline(G, lanes=2)
    with torch.no_grad():
        out = pipe.run(lambda: (delay(), G(**vs[0]))[1])
    if how == "drain":
        pipe.drain()
    else:
        pipe.wait_lane(pipe.last_lane)
    got = {k: out[k].clone() for k in KEYS}
    torch.cuda.synchronize()
    same(got, ref[0])


# ------------------------------------------------------------------------------------------------ 5. first use across lanes
def test_first_use_across_lanes():
    """Weight-derived buffers built on first use (the renderer's packed weight streams and stacked biases, the exact-fp32 stream)
    are shared by all lanes: lane 0 builds them behind a delay, lane 1 reads them at once.  Both views must equal a twin
    generator's serial results -- on a generator that has never run, after an in-place change of a renderer weight (the key
    changes, one lane rebuilds), and after a switch to "fp32_exact" (packed32 is built late).
    (Before the buffers were fenced this passed as well on the box it was tried on -- probably because building a plan uploads
    its tables with copies that block the host until the lane's stream has caught up.  Nothing in the code promised that order.)"""
    from cips_3dplusplus_amd.pipeline import ViewPipeline
    G, twin = G256(11), G256(11)
    nb = noise_for(G, S)
    vs = views(6, 1, seed=41, noise_bufs=nb)
    pipe = ViewPipeline(G, lanes=2)

    def pair(kw0, kw1):
        with torch.no_grad():
            a = pipe.run(lambda: (delay(), G(**kw0))[1], lane=0)
            b = pipe.submit(lane=1, **kw1)
        pipe.drain()
        torch.cuda.synchronize()
        return a, b

    got = pair(vs[0], vs[1])
    ref = serial(twin, vs[:2])
    for i in range(2):
        same(got[i], ref[i], ("fresh", i))

    before = serial(twin, vs[2:3])
    for g_ in (G, twin):                               # (both lanes are warm now; on the caller's stream)
        with torch.no_grad():
            g_.renderer.network.pts_linears[1].weight.mul_(1.25)
    got = pair(vs[2], vs[3])
    ref2 = serial(twin, vs[2:4])
    for i in range(2):
        same(got[i], ref2[i], ("new weights", i))
    assert not torch.equal(ref2[0]["rgb"], before[0]["rgb"])         # (the change does change the image)

    G.set_precision("fp32_exact"); twin.set_precision("fp32_exact")
    got = pair(vs[4], vs[5])
    ref3 = serial(twin, vs[4:6])
    for i in range(2):
        same(got[i], ref3[i], ("fp32_exact", i))


# --------------------------------------------------------------------------------------------------- 6. calls without a plan
@pytest.fixture(scope="module")
def unplanned(gen):
    """A k = 3 generator (no plan at all) and style mixing on the planned one, with their serial references."""
    pkg, configs = _pkg()
    tiny = pkg.build_generator(configs.tiny_G_cfg(32, 2, 3), DEV, seed=6)
    assert tiny._forward_plan(1, 8, N, False) is None
    big, nb, _ = gen
    assert big._forward_plan(1, S, N, False) is not None
    cases = {"k3": (tiny, views(16, 1, seed=51, z_dim=32, img_size=8, noise_bufs=noise_for(tiny, 8))),
             "inject_index": (big, views(16, 1, seed=52, noise_bufs=nb, inject_index=2))}
    return {k: (G, vs, serial(G, vs)) for k, (G, vs) in cases.items()}


@pytest.mark.parametrize("which", ["k3", "inject_index"])
def test_unplanned_forwards_run_one_after_the_other(unplanned, which):
    """(a) Forwards without a plan (k = 3 decoder; style mixing on any generator) write the lane-0 style tables whatever stream they
    are on, so they must not overlap: view 0 sits behind a delay on lane 0 and records an event at its end, view 1 goes to lane 1
    with an event as its first enqueued item.  That item must not start before view 0 has ended.  Deterministic both ways: without
    the ordering lane 1 starts ~20 ms before lane 0's delay is over."""
    from cips_3dplusplus_amd.pipeline import ViewPipeline
    G, vs, ref = unplanned[which]
    pipe = ViewPipeline(G, lanes=2)
    end0, start1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def view0():
        delay()
        out = G(**vs[0])
        end0.record()
        return out

    def view1():
        start1.record()
        return G(**vs[1])

    torch.cuda.synchronize()
    with torch.no_grad():
        a = pipe.run(view0, lane=0)
        b = pipe.run(view1, lane=1)
    pipe.drain()
    torch.cuda.synchronize()
    gap = end0.elapsed_time(start1)
    print(f"{which}: view 1 starts {gap:.3f} ms after view 0 ends")
    assert gap >= 0
    same(a, ref[0], 0)
    same(b, ref[1], 1)


@pytest.mark.parametrize("which", ["k3", "inject_index"])
def test_unplanned_forwards_on_lanes_equal_one_stream(unplanned, which):
    """(b) 16 alternating unplanned views with distinct latents == serial.  On its own this can pass by luck on code that lets
    the two lanes overlap (the tables are small and rewritten early in a forward); the ordering test above is the check that
    cannot."""
    from cips_3dplusplus_amd.pipeline import ViewPipeline
    G, vs, ref = unplanned[which]
    outs = piped(ViewPipeline(G, lanes=2), vs)
    for i in range(len(vs)):
        same(outs[i], ref[i], i)


# --------------------------------------------------------------------------------------------------------------- 7. sequences
@pytest.fixture(scope="module")
def seq_gen():
    G = G256(4)
    g = torch.Generator(device=DEV).manual_seed(9)
    zs = [torch.randn(1, 256, device=DEV, generator=g), torch.randn(1, 256, device=DEV, generator=g)]
    return G, zs, noise_for(G, S, seed=78)


@pytest.mark.parametrize("gather,to_uint8", [(("rgb", "thumb_rgb", "xyz"), False),
                                             (("rgb", "thumb_rgb", "xyz", "normal", "shaded"), False),
                                             (("rgb", "thumb_rgb", "xyz"), True)])
def test_sequences_on_two_lanes_equal_one_lane(seq_gen, gather, to_uint8):
    """sample_multi_view(lanes=2) against lanes=1: the frames, the geometry pass on each lane's own FiLM table, and uint8 frames
    written into the shared block.  The two-lane run comes first, so on a new generator it is also the first use of the
    truncation means."""
    from cips_3dplusplus_amd.multiview import sample_multi_view
    G, zs, nb = seq_gen
    cam_cfg = {"img_size": S, "fov_ang": 6, "dist_radius": 0.12}
    kw = dict(view_mode="yaw", N_frames=5, N_samples=12, noise_bufs=nb, gather=gather, to_uint8=to_uint8)
    two = sample_multi_view(G, cam_cfg, {"static_viewdirs": False}, zs, lanes=2, **kw)
    torch.cuda.synchronize()
    one = sample_multi_view(G, cam_cfg, {"static_viewdirs": False}, zs, lanes=1, **kw)
    torch.cuda.synchronize()
    assert two["rgb"].dtype == (torch.uint8 if to_uint8 else torch.float32) and two["rgb"].shape[0] == 5
    for k in gather:
        assert torch.equal(two[k], one[k]), k
    assert not torch.equal(one["rgb"][0], one["rgb"][1])


# ------------------------------------------------------------------------------------------------------------ 8. book-keeping
def test_lane_streams_and_pipelines_are_shared_and_cached():
    from cips_3dplusplus_amd import pipeline
    pkg, configs = _pkg()
    dev = torch.device("cuda", torch.cuda.current_device())
    a = pipeline.lane_streams(dev, 2)
    b = pipeline.lane_streams(dev, 2)
    assert len(a) == 2 and a[0].cuda_stream != a[1].cuda_stream
    assert a[0] is b[0] and a[1] is b[1]
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=1)
    p1, p2 = pipeline.ViewPipeline(G, 2), pipeline.ViewPipeline(G, 2)
    assert p1 is not p2 and all(x is y for x, y in zip(p1.streams, p2.streams)) and p1.streams[0] is a[0] and p1.streams[1] is a[1]
    p = pipeline.pipeline_for(G, 2)
    assert pipeline.pipeline_for(G, 2) is p and pipeline.pipeline_for(G, 3) is not p and p.G is G
    vs = views(1, 1, seed=61, z_dim=32, img_size=8, noise_bufs=noise_for(G, 8))
    ref = serial(G, vs)
    same(piped(p, vs)[0], ref[0])
    dead = weakref.ref(G)
    del G, p, p1, p2
    gc.collect()
    assert dead() is None                              # the cache is weakly keyed; plans and pipelines do not pin the generator


def test_a_ninth_stream_is_refused_and_the_eight_lanes_stay_usable():
    from cips_3dplusplus_amd import pipeline
    pkg, configs = _pkg()
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=2)
    assert G.MAX_LANES == 8
    vs = views(8, 1, seed=62, z_dim=32, img_size=8, noise_bufs=noise_for(G, 8))
    ref = serial(G, vs)                                # the test's own stream: lane 0
    # torch hands its streams out of a fixed set, round-robin: after this many requests a new one is an old one again, and the
    # pool must still be eight streams of their own (two lanes on one stream would share a plan)
    spent = [torch.cuda.Stream() for _ in range(40)]
    assert len({s.cuda_stream for s in spent}) < 40
    pool = pipeline.lane_streams(torch.device("cuda", torch.cuda.current_device()), 8)
    cur = torch.cuda.current_stream()
    assert len({s.cuda_stream for s in pool} | {cur.cuda_stream}) == 9

    def on(stream, kw):
        stream.wait_stream(cur)
        with torch.cuda.stream(stream), torch.no_grad():
            out = G(**kw)
        cur.wait_stream(stream)
        return out

    for rnd in range(2):
        outs = [on(s, vs[i + 1]) for i, s in enumerate(pool[:7])]
        if rnd == 0:
            assert len(G.__dict__["_stream_lanes"]) == 8
            with pytest.raises(RuntimeError, match="more than 8 different streams"):
                on(pool[7], vs[0])
            torch.cuda.set_stream(cur)
            assert len(G.__dict__["_stream_lanes"]) == 8
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            same(o, ref[i + 1], (rnd, i))
    same(serial(G, vs[:1])[0], ref[0], "lane 0")
