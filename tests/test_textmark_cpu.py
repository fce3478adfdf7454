"""Text watermark (imaginary image.go:322-341, bimg watermarkImageWithText) without a
device: where the planner puts the step and what it refuses, the argument checks of the
per-op entry point and of mipx_submit, the query parameters, the routing of
imaginary.Watermark with a host renderer, and the stand-in renderer itself."""
import ctypes as C

import numpy as np
import pytest

import imaginary_amd as ia
from imaginary_amd import _abi, codec
from imaginary_amd import imaginary as im

L = ia.lib


def _plan(w, h, b, typ="png", **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, b, typ))


def _ops(p):
    return [s[0] for s in p.describe()]


def _code(fn, *a, **kw):
    with pytest.raises(ia.MipxError) as e:
        fn(*a, **kw)
    return e.value.code


# ---------------------------------------------------------------- planner
def test_step_goes_after_blur_and_before_bw():
    p = _plan(400, 300, 3, width=200, sigma=2.0, interpretation=_abi.INTERPRETATION_BW)
    before = _ops(p)
    assert before[-2:] == ["blur", "bw"]
    assert ia.plan_textmark_geometry(p) == (200, 150, 3)      # the post-resize size
    ia.plan_add_textmark(p, 30, 20, 7, 0.5, (1, 128, 254))
    assert _ops(p) == before[:-1] + ["textmark", "bw"]
    name, a, d, out = p.describe()[-2]
    assert a[:6] == (30, 20, 7, 1, 128, 254) and d[0] == 0.5 and out == (200, 150, 3)
    assert (p.out_w, p.out_h, p.out_bands) == (200, 150, 1)
    assert L.mipx_workspace_bytes(C.byref(p), 1) > 0          # the runtime's validation accepts the plan


def test_step_goes_before_the_flatten():
    p = _plan(64, 48, 3, background=(9, 9, 9))
    assert _ops(p) == []
    ia.plan_add_textmark(p, 5, 4, 0, 1.0)
    assert _ops(p) == ["textmark"] and (p.out_w, p.out_h, p.out_bands) == (64, 48, 3)


@pytest.mark.parametrize("given,want", [(0.0, 0.25), (1.7, 1.0), (0.5, 0.5), (1.0, 1.0)])
def test_opacity_default(given, want):
    p = _plan(64, 48, 3)
    ia.plan_add_textmark(p, 5, 4, 3, given)
    assert p.steps[0].d[0] == want


def _validates(plan, mask_shape):
    """The runtime's plan validation (plan_layout) and mask check, without a device:
    mipx_submit runs both before it looks for a running engine."""
    src = np.zeros((plan.in_h, plan.in_w, plan.in_bands), np.uint8)
    dst = np.zeros((plan.out_h, plan.out_w, plan.out_bands), np.uint8)
    mask = np.zeros(mask_shape, np.uint8)
    t = C.c_uint64()
    code = L.mipx_submit(-1, C.byref(plan), C.byref(_img(src)), C.byref(_img(mask)), C.byref(_img(dst)), C.byref(t))
    if code == 0:      # an engine is running in this process: the request is real, let it finish
        assert L.mipx_wait(t.value, -1) == 0
    return code in (0, _abi.MIPX_ENOTINIT)


def test_one_band_image_leaves_with_three_bands():
    p = _plan(64, 48, 1)
    ia.plan_add_textmark(p, 5, 4, 3, 0.5)
    assert (p.out_w, p.out_h, p.out_bands) == (64, 48, 3) and p.steps[0].out_bands == 3
    assert _validates(p, (4, 5, 1))


def test_unsupported_cases():
    for bands in (2, 4):
        assert _code(ia.plan_add_textmark, _plan(64, 48, bands), 5, 4, 3, 0.5) == _abi.MIPX_EUNSUPPORTED
    assert _code(ia.plan_add_textmark, _plan(64, 48, 3), 5, 4, 3, 0.5, (0, 0, 0), True) == _abi.MIPX_EUNSUPPORTED
    wm = ia.plan_make(ia.make_opts(wm_enable=1, wm_opacity=0.5),
                      ia.make_input(64, 48, 3, "png", wm_w=8, wm_h=8, wm_bands=4))
    assert "watermark" in _ops(wm)
    assert _code(ia.plan_add_textmark, wm, 5, 4, 3, 0.5) == _abi.MIPX_EUNSUPPORTED
    twice = _plan(64, 48, 3)
    ia.plan_add_textmark(twice, 5, 4, 3, 0.5)
    assert _code(ia.plan_add_textmark, twice, 5, 4, 3, 0.5) == _abi.MIPX_EUNSUPPORTED
    assert twice.n_steps == 1


def test_one_band_image_with_steps_behind_the_insertion_point():
    """A 1-band image leaves the step with 3 bands, which later steps were not planned
    for.  mipx_plan_make never puts a step behind the insertion point of a 1-band image
    (flatten and B_W need more bands), so the case is a caller's plan: a 1-band image, an
    embed, then a B_W step (1 band in, 1 band out), which the insertion point precedes."""
    g = _plan(64, 48, 1, width=80, height=80, embed=1, enlarge=1)
    assert _ops(g)[-1] == "embed"
    ia.plan_add_textmark(_abi.MipxPlan.from_buffer_copy(g), 5, 4, 3, 0.5)   # nothing behind it: fine
    k = g.n_steps
    g.steps[k].op = _abi.OP_BW
    g.steps[k].out_w, g.steps[k].out_h, g.steps[k].out_bands = g.out_w, g.out_h, 1
    g.n_steps = k + 1
    assert ia.plan_textmark_geometry(g) == (g.out_w, g.out_h, 1)
    assert _code(ia.plan_add_textmark, g, 5, 4, 3, 0.5) == _abi.MIPX_EUNSUPPORTED
    assert g.n_steps == k + 1


def test_add_textmark_argument_checks():
    for args in [(0, 4, 3, 0.5), (5, 0, 3, 0.5), (5, 4, -1, 0.5), (5, 4, 3, 0.5, (0, 256, 0)),
                 (5, 4, 3, 0.5, (-1, 0, 0))]:
        assert _code(ia.plan_add_textmark, _plan(64, 48, 3), *args) == _abi.MIPX_EINVAL
    full = _plan(64, 48, 3)
    full.n_steps = _abi.MAX_STEPS
    assert _code(ia.plan_add_textmark, full, 5, 4, 3, 0.5) in (_abi.MIPX_EINVAL, _abi.MIPX_EUNSUPPORTED)


def test_plan_chain_counts_textmark_as_a_watermark_stage():
    t = _plan(64, 48, 3, sigma=1.0)
    ia.plan_add_textmark(t, 5, 4, 3, 0.5)
    assert _ops(ia.plan_chain([t])) == ["blur", "textmark"]
    assert _ops(ia.plan_chain([_plan(128, 96, 3, width=64), t])) == ["reduce", "blur", "textmark"]
    wm = ia.plan_make(ia.make_opts(wm_enable=1, wm_opacity=0.5),
                      ia.make_input(64, 48, 3, "png", wm_w=8, wm_h=8, wm_bands=3))
    assert "watermark" in _ops(wm)
    assert _code(ia.plan_chain, [t, wm]) == _abi.MIPX_EUNSUPPORTED      # TEXTMARK + WATERMARK stages
    assert _code(ia.plan_chain, [t, t]) == _abi.MIPX_EUNSUPPORTED


def test_plan_validation_of_the_step():
    good = _plan(64, 48, 3)
    ia.plan_add_textmark(good, 5, 4, 3, 0.5)
    assert L.mipx_execute_dev(C.byref(good), 1, 16, 16, None, None, 0, None) == _abi.MIPX_EINVAL   # no mask
    for field, value in [(0, 0), (1, -3), (2, -1), (4, 256)]:
        bad = _abi.MipxPlan.from_buffer_copy(good)
        bad.steps[0].a[field] = value
        assert L.mipx_execute_dev(C.byref(bad), 1, 16, 16, 16, None, 0, None) == _abi.MIPX_EINVAL, (field, value)
    bad = _abi.MipxPlan.from_buffer_copy(good)
    bad.steps[0].out_bands = bad.out_bands = 4
    assert L.mipx_execute_dev(C.byref(bad), 1, 16, 16, 16, None, 0, None) == _abi.MIPX_EINVAL
    alpha = _abi.MipxPlan.from_buffer_copy(good)
    alpha.in_bands = 4
    assert L.mipx_execute_dev(C.byref(alpha), 1, 16, 16, 16, None, 0, None) == _abi.MIPX_EUNSUPPORTED


# ---------------------------------------------------------------- argument checks, no device
def test_per_op_entry_rejects_bad_arguments_before_any_device_call():
    col = (C.c_int32 * 3)(1, 2, 3)

    def call(d_in=16, d_mask=16, d_out=16, n=1, w=8, h=8, b=3, mw=4, mh=4, margin=0, opacity=0.5, colour=col):
        return L.mipx_op_text_watermark(d_in, d_mask, d_out, n, w, h, b, mw, mh, margin, opacity, colour, None)

    for kw in [dict(d_in=None), dict(d_mask=None), dict(d_out=None), dict(colour=None), dict(n=0), dict(margin=-1),
               dict(colour=(C.c_int32 * 3)(0, 256, 0)), dict(colour=(C.c_int32 * 3)(0, 0, -1)), dict(mw=0), dict(mh=0),
               dict(w=0), dict(h=-1), dict(b=0), dict(b=5)]:
        assert call(**kw) == _abi.MIPX_EINVAL, kw
    for bands in (2, 4):
        assert call(b=bands) == _abi.MIPX_EUNSUPPORTED


def _img(a):
    return _abi.MipxImg(a.ctypes.data, a.shape[1], a.shape[0], a.shape[2], a.strides[0])


def test_submit_needs_a_mask_of_the_steps_geometry():
    p = _plan(400, 300, 3, width=256, height=192)
    ia.plan_add_textmark(p, 40, 12, 5, 0.5)
    src = np.zeros((300, 400, 3), np.uint8)
    dst = np.zeros((p.out_h, p.out_w, p.out_bands), np.uint8)
    t = C.c_uint64()
    for shape in [(12, 41, 1), (11, 40, 1), (12, 40, 3), (40, 12, 1)]:
        mask = np.zeros(shape, np.uint8)
        assert L.mipx_submit(-1, C.byref(p), C.byref(_img(src)), C.byref(_img(mask)), C.byref(_img(dst)),
                             C.byref(t)) == _abi.MIPX_EINVAL, shape
    assert L.mipx_submit(-1, C.byref(p), C.byref(_img(src)), None, C.byref(_img(dst)), C.byref(t)) == _abi.MIPX_EINVAL
    # the right mask passes the checks (and finds no engine running: nothing was initialised here)
    mask = np.zeros((12, 40, 1), np.uint8)
    if L.mipx_queue_count() == 0:
        assert L.mipx_submit(-1, C.byref(p), C.byref(_img(src)), C.byref(_img(mask)), C.byref(_img(dst)),
                             C.byref(t)) == _abi.MIPX_ENOTINIT


def test_describe_names_the_op():
    assert _abi.OP_TEXTMARK == 14 and _abi.OP_NAMES[_abi.OP_TEXTMARK] == "textmark"


# ---------------------------------------------------------------- parameters
def test_text_watermark_parameters_parse():
    o = im.build_params_from_query({"margin": "12", "dpi": "96", "textwidth": "300", "font": "sans 12",
                                    "noreplicate": "true", "text": "hi", "color": "1,2,3", "opacity": "0.5"})
    assert (o.margin, o.dpi, o.text_width, o.font, o.no_replicate) == (12, 96, 300, "sans 12", True)
    assert o.is_defined.no_replicate and o.color == [1, 2, 3]
    d = im.build_params_from_query({})
    assert (d.margin, d.dpi, d.text_width, d.font, d.no_replicate) == (0, 0, 0, "", False)
    assert not d.is_defined.no_replicate
    p = im.build_params_from_operation({"params": {"margin": 7, "dpi": 72.0, "textwidth": "50", "noreplicate": False,
                                                   "font": "serif 9"}})
    assert (p.margin, p.dpi, p.text_width, p.font, p.no_replicate) == (7, 72, 50, "serif 9", False)


@pytest.mark.parametrize("query", [{"dpi": "abc"}, {"noreplicate": "maybe"}, {"margin": "1x"}, {"textwidth": "--3"}])
def test_invalid_text_watermark_parameters(query):
    with pytest.raises(im.ImaginaryError):
        im.build_params_from_query(query)


@pytest.mark.parametrize("params", [{"font": 12}, {"noreplicate": 1}, {"margin": True}])
def test_invalid_pipeline_parameter_types(params):
    with pytest.raises(im.ImaginaryError):
        im.build_params_from_operation({"params": params})


# ---------------------------------------------------------------- Watermark routing
def _fake_run(calls):
    def run(plan, px, wm):
        calls.append((plan, px.shape, wm))
        return np.zeros((plan.out_h, plan.out_w, plan.out_bands), np.uint8)
    return run


def test_watermark_renders_with_the_go_defaults_and_hands_the_mask_over(monkeypatch):
    calls, asked = [], []
    monkeypatch.setattr(im, "_run", _fake_run(calls))
    mask = np.arange(7 * 23, dtype=np.uint8).reshape(7, 23)

    def render(text, font, width, dpi):
        asked.append((text, font, width, dpi))
        return mask

    img = im.Decoded(np.zeros((300, 400, 3), np.uint8), type="png")
    o = im.build_params_from_query({"text": "hello", "width": "250", "color": "9,8,7"})
    out = im.Watermark(img, o, render=render)
    assert asked == [("hello", "sans 10", 250 // 6, 150)]
    assert out.shape == (188, 250, 3) and len(calls) == 1
    plan, shape, wm = calls[0]
    assert shape == (300, 400, 3)
    assert _ops(plan)[-1] == "textmark" and _ops(plan)[:-1] == _ops(_plan(400, 300, 3, width=250, force=1))
    s = plan.steps[plan.n_steps - 1]
    assert tuple(s.a[:6]) == (23, 7, 250 // 6, 9, 8, 7) and s.d[0] == 0.25     # margin 0 -> the text width
    assert wm.shape == (7, 23, 1) and np.array_equal(wm[:, :, 0], mask)
    # without a renderer the operation stays with libvips, as before
    for kw in ({}, {"render": None}):
        with pytest.raises(im.EngineUnsupported):
            im.Watermark(img, o, **kw)
    with pytest.raises(im.ImaginaryError) as e:
        im.Watermark(img, im.build_params_from_query({}), render=render)
    assert not isinstance(e.value, im.EngineUnsupported) and "text" in e.value.message
    assert len(calls) == 1 and len(asked) == 1


def test_watermark_passes_explicit_parameters_through(monkeypatch):
    calls, asked = [], []
    monkeypatch.setattr(im, "_run", _fake_run(calls))
    img = im.Decoded(np.zeros((60, 80, 1), np.uint8), type="png")
    o = im.build_params_from_query({"text": "a b", "textwidth": "33", "dpi": "96", "font": "sans 12", "margin": "5",
                                    "opacity": "0.7", "color": "1,2"})
    im.Watermark(img, o, render=lambda *a: asked.append(a) or np.ones((3, 4), np.uint8))
    assert asked == [("a b", "sans 12", 33, 96)]
    plan = calls[0][0]
    s = plan.steps[plan.n_steps - 1]
    assert tuple(s.a[:6]) == (4, 3, 5, 0, 0, 0)            # fewer than three colour values: black (image.go:336)
    assert s.d[0] == float(np.float32(0.7)) and plan.out_bands == 3


def test_watermark_fallback_cases(monkeypatch):
    calls, rendered = [], []
    monkeypatch.setattr(im, "_run", _fake_run(calls))
    render = lambda *a: rendered.append(a) or np.ones((3, 4), np.uint8)   # noqa: E731
    rgba = im.Decoded(np.zeros((60, 80, 4), np.uint8), type="png")
    with pytest.raises(im.EngineUnsupported):
        im.Watermark(rgba, im.build_params_from_query({"text": "x"}), render=render)
    rgb = im.Decoded(np.zeros((60, 80, 3), np.uint8), type="png")
    with pytest.raises(im.EngineUnsupported):
        im.Watermark(rgb, im.build_params_from_query({"text": "x", "noreplicate": "true"}), render=render)
    assert len(rendered) == 1 and not calls                 # noreplicate is refused before rendering


def test_pipeline_hands_the_renderer_to_watermark_stages_only(monkeypatch):
    calls, asked = [], []
    monkeypatch.setattr(im, "_run", _fake_run(calls))
    mask = np.full((5, 9), 200, np.uint8)
    ops = [{"operation": "resize", "params": {"width": 120}},
           {"operation": "watermark", "params": {"text": "pipeline", "margin": 3}},
           {"operation": "blur", "params": {"sigma": 1.5}}]
    img = im.Decoded(np.zeros((120, 160, 3), np.uint8), type="png")
    out = im.Pipeline(img, im.build_params_from_query({"operations": ops}),
                      render=lambda *a: asked.append(a) or mask)
    assert asked == [("pipeline", "sans 10", 20, 150)]       # the stage's own input: 120 wide
    assert out.shape == (90, 120, 3) and len(calls) == 1
    plan, _, wm = calls[0]
    assert _ops(plan) == ["reduce", "textmark", "blur"]
    assert np.array_equal(wm[:, :, 0], mask)


# ---------------------------------------------------------------- the stand-in renderer
def test_render_text_gives_a_tight_mask():
    try:
        m = codec.render_text("imaginary on the engine, wrapped over lines", "sans 10", 120, 150)
    except codec.CodecError as e:
        pytest.skip(f"no text renderer here: {e}")
    assert m.ndim == 2 and m.dtype == np.uint8 and m.size > 0
    assert m.shape[1] <= 120
    assert m.max() > 0 and m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()   # tight
    one = codec.render_text("imaginary", "sans 10", 0, 150)
    big = codec.render_text("imaginary", "sans 20", 0, 150)
    assert big.shape[0] > one.shape[0] and big.shape[1] > one.shape[1]
    assert m.shape[0] > one.shape[0]                          # wrapped: more than one line
