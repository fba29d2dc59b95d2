"""The trunk layer issues the same libavt launches, with the same arguments, as the commit that recorded
tests/golden/launch_traces.json: every ``call`` and ``query`` that trunk.py, tube.py and engine.py make while an engine is
built and run, in order.  The library's entry points decide every kernel and plan from their scalar arguments, so an
equal trace on an unchanged library means the same kernels on the same geometries; which tensor a pointer names is
what the forced-tape tests hold.

A record is [entry name, arg, arg, ...]: integers and floats by value (ctypes scalars by their ``.value``), every
pointer -- a tensor's address, a stream, a ``byref`` struct, a ctypes array -- as 0 (null) or 1.  The default stream is
the null stream, so a launch on the side stream shows as a 1 in the last place.  The fixture holds each distinct record
once and, per case, the list of their indices.

Each case builds its engine inside the recording (the weight-pack and fold descriptor tables are part of the trace)
and starts from an empty gather-table cache (trunk._PIXTABS), so a trace does not depend on which tests ran before; the
tables it registers stay alive in the cache afterwards.  ``run_case`` also returns the tensors a case produced
(outputs, the flat gradient, running statistics, batch counters) for a bitwise comparison of two trees."""
import contextlib
import ctypes
import json
import os

import pytest
import torch

import avenet_oracle as orc
import tube_oracle as tor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")
TUBE_CASES = [(1, False), (3, True)]  # tests/test_tube_e2e_gpu.py's CASES: (t, one spectrogram per clip)
VIDEOS = {"v2x4x32x32": (2, 3, 4, 32, 32), "v1x3x17x9": (1, 3, 3, 17, 9)}


def _arg(a):
    if a is None:
        return 0
    if isinstance(a, (bool, int)):
        return int(a)
    if isinstance(a, float):
        return a
    if isinstance(a, ctypes.c_void_p):
        return int(bool(a.value))
    if isinstance(a, ctypes._SimpleCData):  # c_float, c_int, c_longlong by value
        return a.value
    return 1  # byref(struct), a ctypes array: a pointer that is not null


@contextlib.contextmanager
def recording():
    """Replace ``call`` and ``query`` in trunk, tube and engine with wrappers that append a record and pass through;
    yields the list."""
    import avt_amd.engine
    import avt_amd.trunk
    import avt_amd.tube

    records, saved = [], []

    def wrap(orig):
        def f(entry, *args):
            records.append([entry] + [_arg(a) for a in args])
            return orig(entry, *args)
        return f

    torch.cuda.synchronize()
    tabs = avt_amd.trunk._PIXTABS
    avt_amd.trunk._PIXTABS = {}
    for mod in (avt_amd.trunk, avt_amd.tube, avt_amd.engine):
        for name in ("call", "query"):
            saved.append((mod, name, getattr(mod, name)))
            setattr(mod, name, wrap(getattr(mod, name)))
    try:
        yield records
    finally:
        for mod, name, orig in saved:
            setattr(mod, name, orig)
        torch.cuda.synchronize()
        tabs.update(avt_amd.trunk._PIXTABS)  # the tables registered last are the ones the library reads
        avt_amd.trunk._PIXTABS = tabs


def _state(flat, **out):
    out.update(bflat=flat.bflat, nbt=flat.nbt)
    return {k: v for k, v in out.items() if v is not None}


# ------------------------------------------------------------------------------------------------ AVEngine
def _avenet():
    from avt_amd.model import AVENet

    m = AVENet(orc.Args(), False)
    m.load_state_dict(orc.make_state(0))
    m = m.to(DEV)
    eng = m.engine()
    eng._keep = m  # (the flat store binds the module)
    return eng, orc.make_image(2, 64).to(DEV), orc.make_spectrogram(2, 65, 76).to(DEV)


def _av_train(fuse=False, defer=False):
    import avt_amd.trunk

    old = avt_amd.trunk.FUSE_BN_BWD
    avt_amd.trunk.FUSE_BN_BWD = fuse
    try:
        eng, img, aud = _avenet()
        eng.defer_wgrad = defer
        out, tape = eng.forward(img, aud, True, with_ce=True)
        tape["img"]["want_dx"] = tape["aud"]["want_dx"] = True
        gflat = torch.zeros(eng.flat.n_train, device=DEV, dtype=torch.float32)
        eng.backward(tape, out["dlogits"], gflat)
    finally:
        avt_amd.trunk.FUSE_BN_BWD = old
    return _state(eng.flat, gflat=gflat, dx_img=tape["img"]["dx"], dx_aud=tape["aud"]["dx"],
                  **{k: out[k] for k in ("A", "logits", "weighted_A", "Pos", "Neg", "loss", "dlogits")})


def _av_eval(frozen):
    eng, img, aud = _avenet()
    out, tape = eng.forward(img, aud, False, tape=True)
    for k in ("img", "aud"):
        tape[k]["want_dx"], tape[k]["frozen"] = True, frozen
    dlogits = torch.randn(out["logits"].shape, generator=torch.Generator().manual_seed(23)).to(DEV)
    gflat = None if frozen else torch.zeros(eng.flat.n_train, device=DEV, dtype=torch.float32)
    eng.backward(tape, dlogits, gflat)
    return _state(eng.flat, gflat=gflat, dx_img=tape["img"]["dx"], dx_aud=tape["aud"]["dx"], A=out["A"],
                  logits=out["logits"], weighted_A=out["weighted_A"])


def _av_folded():
    eng, img, aud = _avenet()
    out, _ = eng.forward_folded(img, aud, layer_io=True)
    return _state(eng.flat, **{k: out[k] for k in ("A", "logits", "weighted_A", "Pos", "Neg", "v", "v_in", "a", "a_in")})


# ------------------------------------------------------------------------------------------------ TrunkEngine
def _trunk(modal):
    """test_trunk2d_backward_forced_gpu.py's sizes: forward, backward with the input gradient, the folded forward."""
    from avt_amd.model import resnet18

    sd = orc.make_state(0)
    prefix = "audnet." if modal == "audio" else "imgnet."
    net = resnet18(modal=modal)
    net.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    net = net.to(DEV).train()
    eng, flat, _, _ = net._engine_and_params()
    if modal == "audio":
        x, g_out = orc.make_spectrogram(2, 65, 76), orc.make_gout(2, 5, 5)
    else:
        x, g_out = orc.make_image(3, 64), orc.make_gout(3, 4, 4)
    y, tp = eng.forward(x.to(DEV), True)
    tp["want_dx"] = True
    gflat = torch.zeros(flat.n_train, device=DEV, dtype=torch.float32)
    dx = eng.backward(tp, g_out.to(DEV), gflat)
    yf = eng.forward_folded(x.to(DEV))
    return _state(flat, y=y, gflat=gflat, dx=dx, folded=yf)


# ------------------------------------------------------------------------------------------------ TubeEngine
def _tube(video_backward, t, per_clip):
    """test_tube_e2e_gpu.py's sizes: the train step's forward and backward, then the folded forward."""
    from avt_amd.model import FullModel

    m = FullModel(orc.Args())
    m.load_state_dict(tor.make_tube_state(0))
    m = m.to(DEV).train()
    if video_backward:
        m.enable_video_backward()
    spec = orc.make_spectrogram(2, 65, 76)
    audio = (spec if per_clip else tor.repeat_spectrogram(spec, t)).to(DEV)
    video = tor.make_video(2, t, 64).to(DEV)
    eng = m.engine()
    assert eng.video_backward == video_backward
    out, tape = eng.forward(audio, video, True, with_ce=True)
    gflat = torch.zeros(eng.flat.n_train, device=DEV, dtype=torch.float32)
    eng.backward(tape, out["dlogits"], gflat)
    outf, _ = eng.forward_folded(audio, video)
    return _state(eng.flat, gflat=gflat, A=out["A"], logits=out["logits"], loss=out["loss"], v=out["v"],
                  folded_A=outf["A"], folded_logits=outf["logits"])


# ------------------------------------------------------------------------------------------------ R3DEngine
def _r3d(max_pool, vshape):
    """A forward-only engine (train forward, eval forward, folded forward), then one with the backward on the same
    store: the train tape and the eval-grad tape, each with backward(..., want_gvideo=True)."""
    from avt_amd.resnet3D import generate_model
    from avt_amd.tube import R3DEngine

    sd = tor.make_tube_state(0)
    net = generate_model(18, no_max_pool=not max_pool, n_classes=1039)
    net.load_state_dict({k[len("vidnet."):]: v for k, v in sd.items() if k.startswith("vidnet.")})
    net.enable_backward()
    net = net.to(DEV).train()
    flat = net._flat_store()
    b = vshape[0]
    video = torch.randn(vshape, generator=torch.Generator().manual_seed(5)).to(DEV)
    glogits = tor.make_glogits(b).float().to(DEV)
    e0 = R3DEngine(flat, "", max_pool=max_pool)
    out = {"fwd_train": e0.forward(video, True), "fwd_eval": e0.forward(video, False),
           "folded": e0.forward_folded(video)}
    e1 = R3DEngine(flat, "", max_pool=max_pool, with_backward=True)
    for tag, training in (("train", True), ("eval", False)):
        logits, tp = e1.forward(video, training, tape=True, input_grad=True)
        gflat = torch.zeros(flat.n_train, device=DEV, dtype=torch.float32)
        gvideo = e1.backward(tp, glogits, gflat, want_gvideo=True)
        out.update({f"{tag}_logits": logits, f"{tag}_gflat": gflat, f"{tag}_gvideo": gvideo})
    return _state(flat, **out)


CASES = {
    "avengine-train": lambda: _av_train(),
    "avengine-train-fused-bn-bwd": lambda: _av_train(fuse=True),
    "avengine-train-defer-wgrad": lambda: _av_train(defer=True),
    "avengine-eval-tape": lambda: _av_eval(False),
    "avengine-eval-tape-frozen": lambda: _av_eval(True),
    "avengine-folded": _av_folded,
    "trunkengine-vision": lambda: _trunk("vision"),
    "trunkengine-audio": lambda: _trunk("audio"),
}
for _vb in (False, True):
    for _t, _pc in TUBE_CASES:
        CASES[f"tubeengine-{'e2e' if _vb else 'detached'}-t{_t}-{'perclip' if _pc else 'folded'}"] = \
            lambda vb=_vb, t=_t, pc=_pc: _tube(vb, t, pc)
for _mp in (False, True):
    for _vn, _vs in VIDEOS.items():
        CASES[f"r3dengine-{'maxpool' if _mp else 'nopool'}-{_vn}"] = lambda mp=_mp, vs=_vs: _r3d(mp, vs)


def run_case(name):
    """(the case's records, {tensor name: tensor}) from fixed seeds."""
    with recording() as records:
        tensors = CASES[name]()
        torch.cuda.synchronize()
    return records, tensors


_GOLDEN = {}


def _golden(name):
    if not _GOLDEN:
        with open(GOLDEN) as f:
            _GOLDEN.update(json.load(f))
    return [_GOLDEN["records"][i] for i in _GOLDEN["cases"][name]]


@pytest.mark.parametrize("name", list(CASES))
def test_same_launches(name):
    """The case's records equal the fixture's, one by one and in order."""
    want = _golden(name)
    got, tensors = run_case(name)
    for t in tensors.values():
        assert bool(torch.isfinite(t.float()).all())
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: record {i} of {len(want)}: {g} != recorded {w} (after {got[max(0, i - 3):i]})"
    n = min(len(got), len(want))
    assert len(got) == len(want), f"{name}: {len(got)} records, {len(want)} recorded; the first one without a " \
                                  f"partner: {max(got, want, key=len)[n]}"
