"""The one-call forward launches what the route resolver says (csrc/decoder_route.hip), and refuses a plan whose flags promise
something else before it enqueues anything."""
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import _lib, configs, hip, plan as plan_mod
from cips_3dplusplus_amd.camera import Camera

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_SAMPLES = 8


def _generator(res, precision):
    G = pkg.build_generator(configs.ffhq_G_cfg(res, 2), DEV, seed=0)
    G.set_precision(precision)
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=torch.zeros(1, 2, device=DEV))
    g = torch.Generator(device=DEV).manual_seed(res)
    kw = dict(zs=[torch.randn(1, 256, device=DEV, generator=g), torch.randn(1, 256, device=DEV, generator=g)], cam_poses=e, focals=f,
              img_size=64, near=n, far=fa, nerf_cfg=dict(N_samples=N_SAMPLES, perturb=False, static_viewdirs=False))
    return G, kw


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("res", [256, 1024])
def test_forward_marks_are_the_step_list(res, precision):
    G, kw = _generator(res, precision)
    marks = hip.DecoderMarks(96)
    hip.DECODER_MARKS = marks
    G(**kw)
    torch.cuda.synchronize()
    pl = G._forward_plan(1, 64, N_SAMPLES, False)
    steps = pl.steps()
    recorded = [[marks.info[4 * k + j] for j in range(4)] for k in range(marks.count.value)]
    assert recorded[:2] == [[0, 0, 0, 0], [0, 0, 0, 0]]                  # the two START marks in front of the first launch
    assert recorded[2:] == [list(s.mark) for s in steps if s.mark[0] >= 0]
    assert len(recorded) - 2 == len(steps) - sum(1 for s in steps if s.form & 64 and s.kind == _lib.STEP_KINDS.index("flush"))
    assert pl.u8_capable and steps[-1].kind == _lib.STEP_FUSED_STAGE


def test_broken_plan_is_refused_before_anything_is_enqueued():
    """CIPS3D_DEC_CHAINED on the first up-sampling conv, whose low-resolution GEMM no earlier stage computes: the forward returns
    CIPS3D_E_BADARG, and neither the style tables (the first thing a forward writes) nor the image were touched."""
    G, kw = _generator(256, "fp32")
    G(**kw)                                                              # builds the plan; a full, valid forward
    pl = G._forward_plan(1, 64, N_SAMPLES, False)
    good = pl.plan
    broken = plan_mod.GeneratorPlan.from_buffer_copy(good)
    head = next(i for i in range(good.n_dec_layers) if good.layers[i].kind == 1)
    assert not broken.layers[head].flags & _lib.DEC_CHAINED
    broken.layers[head].flags |= _lib.DEC_CHAINED
    rgb = torch.empty(1, 3, pl.out_res, pl.out_res, device=DEV)
    watched = [rgb, pl.styles_r, pl.styles_d, pl.film, pl.s_buf]
    SENTINEL = 12345.0
    for t in watched:
        t.fill_(SENTINEL)
    torch.cuda.synchronize()
    pl.plan = broken
    try:
        with pytest.raises(RuntimeError, match=r"cips3d_generator_forward failed \(-1\)"):
            G(rgb_out=rgb, **kw)
    finally:
        pl.plan = good
    torch.cuda.synchronize()
    for t in watched:
        assert bool((t == SENTINEL).all())
    # the same call on the plan as built runs
    out = G(rgb_out=rgb, **kw)["rgb"]
    torch.cuda.synchronize()
    assert out.data_ptr() == rgb.data_ptr() and bool(torch.isfinite(rgb).all()) and not bool((rgb == SENTINEL).any())
