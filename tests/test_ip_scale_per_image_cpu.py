"""CPU: the per-batch-item IP-Adapter scale, everything that needs no device.

  * ``tg_attention_ps`` / ``tg_rc_xattn_ps`` / ``tg_xq_attn_ps`` are declared in the header with the UNCHANGED descriptors plus ``int32_t ip_scale_count``,
    bound in ``_lib.SIGNATURES`` with that argument list and exported by the library; the ABI stays 308 and the three descriptors keep their sizes;
  * each of them refuses, on the host and before any launch, a count that is neither 0, 1 nor the launch's batch, and a per-item count with a null scale
    pointer (``TG_ERR_ARG`` + ``tg_last_error``);
  * ``IPAttnProcessor.scale``: a number reads back as assigned, a vector as a tuple of floats, ``named_parameters()`` is what it was;
  * ``pipelines.generate_characters`` refuses ``'xl'`` and a duplicated new ``obj_id`` (stubs: no device, no model);
  * ``story.story_jobs(ip_scales=)``.
"""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TG_ERR_ARG = -1
FAKE = 16                                                             # a non-null, 16-byte aligned "pointer": validation never reads it
# ctypes.sizeof of tg_attn_desc / tg_rc_xattn_desc / tg_xq_attn_desc at the parent commit (ABI 308)
DESC_SIZES = {"AttnDesc": 240, "RcXattnDesc": 96, "XqAttnDesc": 120}
NEW = {"tg_attention_ps": ("tg_attention", "tg_attn_desc", "AttnDesc"), "tg_rc_xattn_ps": ("tg_rc_xattn", "tg_rc_xattn_desc", "RcXattnDesc"),
       "tg_xq_attn_ps": ("tg_xq_attn", "tg_xq_attn_desc", "XqAttnDesc")}


def _lib_built():
    from theatergen_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_symbols_are_declared_bound_and_exported_at_abi_308():
    _lib = _lib_built()
    header = open(os.path.join(ROOT, "include", "theatergen_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, (old, desc, cls) in NEW.items():
        assert re.search(rf"^int {name}\(const {desc}\* d, int32_t ip_scale_count, void\* stream\);", header, flags=re.M), f"{name} is not declared"
        at = header.index(f"int {name}(")
        assert "Additive to ABI 308" in header[header.rindex("/*", 0, at):at], f"{name}: no 'Additive to ABI 308' note on its declaration"
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.i32 and len(args) == 3 and args[0] is C.POINTER(getattr(_lib, cls)) and args[1] is _lib.i32 and args[2] is _lib.vp
        assert _lib.SIGNATURES[old] == (res, [args[0], args[2]]), f"{old} lost its signature"
        assert re.search(rf"\bT {name}$", nm, flags=re.M), f"libtheatergen_hip.so does not export {name}"
        assert getattr(_lib.lib(), name) is not None
    assert re.search(r"#define TG_ABI_VERSION 308\b", header) and _lib.ABI_VERSION == 308 and _lib.lib().tg_version() == 308


def test_descriptor_layouts_are_the_parents():
    from theatergen_amd import _lib
    for cls, size in DESC_SIZES.items():
        assert C.sizeof(getattr(_lib, cls)) == size, f"{cls}: {C.sizeof(getattr(_lib, cls))} bytes, the parent's is {size}"
    assert _lib.AttnDesc.w1_dev.offset == 200 and _lib.RcXattnDesc.ip_scale.offset == 88 and _lib.XqAttnDesc.ip_scale.offset == 64


def _attn_desc(batch=3, w1_dev=FAKE):
    from theatergen_amd import _lib
    d = _lib.AttnDesc()
    heads, hd, n_q, len0, len1 = 2, 40, 160, 77, 4
    inner = heads * hd
    d.dtype, d.batch, d.heads, d.head_dim, d.n_q, d.len0, d.len1 = 0, batch, heads, hd, n_q, len0, len1
    d.q = d.k0 = d.vt0 = d.k1 = d.vt1 = d.out = FAKE
    d.q_ld, d.q_bs, d.k0_ld, d.k0_bs, d.vt0_ld, d.vt0_bs = inner, n_q * inner, inner, len0 * inner, 80, inner * 80
    d.k1_ld, d.k1_bs, d.vt1_ld, d.vt1_bs = inner, len1 * inner, 8, inner * 8
    d.out_ld, d.out_bs, d.scale = inner, n_q * inner, hd ** -0.5
    d.w1_dev = w1_dev
    return d


def _rc_desc(batch=3, ip_scale=FAKE):
    from theatergen_amd import _lib
    d = _lib.RcXattnDesc()
    d.dtype, d.h, d.ldh, d.wq, d.kv, d.wo, d.out, d.ldc = 0, FAKE, 320, FAKE, FAKE, FAKE, FAKE, 320
    d.M, d.rows_per_batch, d.text_len, d.ip_tokens, d.ln_eps, d.ip_scale = batch * 128, 128, 77, 4, 1e-5, ip_scale
    return d


def _xq_desc(batch=3, ip_scale=FAKE):
    from theatergen_amd import _lib
    d = _lib.XqAttnDesc()
    d.dtype, d.x, d.ldx, d.wq, d.ln_u, d.ln_v, d.ln_eps, d.kv, d.ip_scale = 0, FAKE, 640, FAKE, FAKE, FAKE, 1e-5, FAKE, ip_scale
    d.out, d.ldc, d.M, d.C, d.head_dim, d.rows_per_batch, d.text_len, d.ip_tokens = FAKE, 640, batch * 128, 640, 80, 128, 77, 4
    return d


@pytest.mark.parametrize("name,desc", [("tg_attention_ps", _attn_desc), ("tg_rc_xattn_ps", _rc_desc), ("tg_xq_attn_ps", _xq_desc)])
def test_bad_counts_are_refused_before_any_launch(name, desc):
    """batch 3: every count other than 0, 1 and 3 is TG_ERR_ARG, and so is 3 with a null scale pointer.  The descriptors are otherwise valid and their
    pointers fake: a call that got as far as a launch would not come back with TG_ERR_ARG and this entry point's message."""
    h = _lib_built().lib()
    fn = getattr(h, name)
    for count in (2, 4, 6, -1, -3, 1 << 20):
        assert h.tg_gemm(C.byref(_lib_built().GemmDesc()), None) == -1 and b"tg_gemm" in h.tg_last_error()      # another call's message, to be replaced
        assert fn(C.byref(desc()), count, None) == TG_ERR_ARG, f"{name}: count {count} at batch 3"
        assert name.encode() in h.tg_last_error() and b"ip_scale_count" in h.tg_last_error(), h.tg_last_error()
    assert fn(C.byref(desc(ip_scale=None) if name != "tg_attention_ps" else desc(w1_dev=None)), 3, None) == TG_ERR_ARG
    assert name.encode() in h.tg_last_error() and b"needs" in h.tg_last_error(), h.tg_last_error()
    assert fn(None, 0, None) == TG_ERR_ARG


def test_processor_scale_attribute_number_and_vector():
    from theatergen_amd.attention_processor import IPAttnProcessor
    p = IPAttnProcessor(64, 32, scale=0.4, num_tokens=4)
    names = [n for n, _ in p.named_parameters()]
    assert names == ["to_k_ip.weight", "to_v_ip.weight"] and not list(p.named_buffers())
    assert p.scale == 0.4 and type(p.scale) is float
    p.scale = 0                                                        # the reference assigns the int 0 for a first appearance
    assert p.scale == 0 and type(p.scale) is int
    t0 = torch.tensor(0.25)
    p.scale = t0                                                       # a 0-d tensor is a number: kept as assigned
    assert p.scale is t0
    for vec in ([0.0, 0.4, 1.7], (0.0, 0.4, 1.7), torch.tensor([0.0, 0.4, 1.7]), torch.tensor([0.0, 0.4, 1.7], dtype=torch.float64).numpy()):
        p.scale = vec
        assert isinstance(p.scale, tuple) and len(p.scale) == 3 and all(type(v) is float for v in p.scale)
        assert p.scale == pytest.approx((0.0, 0.4, 1.7))
        assert p.scale_count(3) == 3 and p.scale_count(6) == 1
    assert [n for n, _ in p.named_parameters()] == names and not list(p.named_buffers())
    for bad in ([], [[0.1, 0.2]], torch.zeros(2, 2)):
        with pytest.raises(ValueError):
            p.scale = bad
    assert p.scale == pytest.approx((0.0, 0.4, 1.7)), "a refused assignment must leave the scale alone"
    p.scale = 0.7
    assert p.scale == 0.7 and not p._scale_bufs and p.scale_count(3) == 1              # no device buffer was ever made


def test_scale_buffers_are_never_replaced_and_every_assignment_writes_all_of_them():
    """one buffer per (device, length), made on first use and kept: a captured graph holds its address.  A number fills every buffer; a vector goes into
    the buffer of its length and poisons the others (a graph captured with another count must not replay a plausible stale value)"""
    import math
    from theatergen_amd.attention_processor import IPAttnProcessor
    cpu = torch.device("cpu")
    p = IPAttnProcessor(64, 32, scale=0.4, num_tokens=4)
    one = p.scale_device(cpu, 4)
    assert one.tolist() == pytest.approx([0.4]) and p.scale_count(4) == 1
    p.scale = [0.0, 0.4, 0.0, 0.4]
    assert math.isnan(one.item()) and p.scale_count(4) == 4
    four = p.scale_device(cpu, 4)
    assert four is not one and four.tolist() == pytest.approx([0.0, 0.4, 0.0, 0.4]) and p.scale_device(cpu, 4) is four
    with pytest.raises(ValueError, match=r"4 per-batch-item values.*batch 6"):
        p.scale_device(cpu, 6)
    p.scale = [0.1] * 6                                                # another length: a THIRD buffer, the first two stay where they are
    six = p.scale_device(cpu, 6)
    assert six.tolist() == pytest.approx([0.1] * 6) and all(math.isnan(v) for v in four.tolist() + one.tolist())
    assert p.scale_device(cpu, 6) is six and set(p._scale_bufs) == {(cpu, 1), (cpu, 4), (cpu, 6)}
    p.scale = [0.5, 0.6, 0.7, 0.8]                                     # back to length 4: the SAME [4] buffer, rewritten
    assert p.scale_device(cpu, 4) is four and four.tolist() == pytest.approx([0.5, 0.6, 0.7, 0.8]) and math.isnan(six[0].item())
    p.scale = 0.3                                                      # a number fills all three; calls of batch 4 / 6 keep reading their [n] buffer
    assert one.tolist() == pytest.approx([0.3]) and four.tolist() == pytest.approx([0.3] * 4) and six.tolist() == pytest.approx([0.3] * 6)
    assert p.scale_device(cpu, 4) is four and p.scale_device(cpu, 6) is six and p.scale_device(cpu, 8) is one and p.scale_device(cpu) is one
    assert (p.scale_count(4), p.scale_count(6), p.scale_count(8), p.scale_count(1)) == (4, 6, 1, 1)


def test_engine_signature_and_graphed_grad_look_at_the_scale_form():
    """the two owners of captured graphs: ``DenoiseEngine._signature`` carries the count per processor and refuses a vector of another engine's length;
    ``_check_replayable`` (after a before_step hook) and ``GraphedInputGrad.run`` raise when the form moved since the capture"""
    from theatergen_amd import backward
    from theatergen_amd.attention_processor import IPAttnProcessor
    from theatergen_amd.pipelines import DenoiseEngine
    procs = {"a": IPAttnProcessor(64, 32, scale=0.4), "b": IPAttnProcessor(64, 32, scale=0.4)}
    unet = types.SimpleNamespace(attn_processors=procs)
    eng = types.SimpleNamespace(unet=unet, n_img=2, frozen=None, frozen_steps=0, g=7.5, use_graph=True, _ip_processors=lambda: list(procs.values()))
    eng._signature = lambda: DenoiseEngine._signature(eng)
    eng._graph_sig = eng._signature()
    assert eng._graph_sig[-1] == (1, 1)
    DenoiseEngine._check_replayable(eng)
    for p in procs.values():
        p.scale = 0.0                                                  # new VALUE: same signature
    DenoiseEngine._check_replayable(eng)
    procs["b"].scale = [0.0, 0.4, 0.0, 0.4]                            # what a hook would do: per-image values on a step captured with a number
    assert eng._signature()[-1] == (1, 4)
    with pytest.raises(RuntimeError, match="before_step hook changed"):
        DenoiseEngine._check_replayable(eng)
    procs["b"].scale = [0.1] * 6                                       # another engine's length
    with pytest.raises(ValueError, match=r"6 per-batch-item scales.*batch 4"):
        DenoiseEngine._check_replayable(eng)
    procs["b"].scale = 0.4
    DenoiseEngine._check_replayable(eng)
    # GraphedInputGrad.run: the check comes before anything is copied or replayed
    assert backward.ip_scale_forms(unet) == (0, 0)
    gig = types.SimpleNamespace(unet=unet, _ip_forms=backward.ip_scale_forms(unet))
    procs["a"].scale = [0.0, 0.4]
    assert backward.ip_scale_forms(unet) == (2, 0)
    with pytest.raises(RuntimeError, match="form of an IPAttnProcessor.scale changed"):
        backward.GraphedInputGrad.run(gig)


def test_host_constant_paths_refuse_a_vector():
    from theatergen_amd.attention_processor import IPAttnProcessor, host_ip_scale
    p = IPAttnProcessor(64, 32, scale=0.4, num_tokens=4)
    assert host_ip_scale(p, "x") == 0.4
    p.scale = [0.9, 0.1]
    with pytest.raises(NotImplementedError, match="2 per-batch-item"):
        host_ip_scale(p, "the attention reverse pass")


def test_ops_refuse_other_lengths_before_the_library(monkeypatch):
    """1 or ``batch`` elements: ops raises RuntimeError itself for any other length (the library is never asked: it is made unreachable here)"""
    from theatergen_amd import _lib, ops
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("ops called into the library")))
    fake = types.SimpleNamespace(dtype=torch.float32, is_cuda=True, is_contiguous=lambda: True, numel=lambda: 2)
    for batch in (3, 4):
        with pytest.raises(RuntimeError, match="2 elements"):
            ops._ip_scale_count(fake, batch, "attention")
    assert ops._ip_scale_count(fake, 2, "attention") == 2 and ops._ip_scale_count(None, 2, "attention") == 0
    with pytest.raises(RuntimeError):
        ops._ip_scale_count(torch.zeros(3, dtype=torch.float32), 3, "attention")                 # not on the device
    with pytest.raises(RuntimeError):
        ops._ip_scale_count(types.SimpleNamespace(dtype=torch.float16, is_cuda=True, is_contiguous=lambda: True, numel=lambda: 3), 3, "attention")


def test_engine_and_adapter_hand_the_scales_to_the_processors():
    """``IPAdapter.set_scale`` passes a sequence on unchanged; ``DenoiseEngine.set_ip_scale`` writes [s ; s] (unconditional half first) or the number"""
    from theatergen_amd.attention_processor import IPAttnProcessor
    from theatergen_amd.ip_adapter import IPAdapter
    from theatergen_amd.pipelines import DenoiseEngine
    procs = {"a": IPAttnProcessor(64, 32, scale=1.0), "b": IPAttnProcessor(64, 32, scale=1.0), "c": object()}
    unet = types.SimpleNamespace(attn_processors=procs)
    IPAdapter.set_scale(types.SimpleNamespace(pipe=types.SimpleNamespace(unet=unet)), [0.0, 0.4, 0.0, 0.4])
    assert procs["a"].scale == procs["b"].scale == (0.0, 0.4, 0.0, 0.4)
    eng = types.SimpleNamespace(unet=unet, n_img=3, _ip_processors=lambda: [p for p in procs.values() if isinstance(p, IPAttnProcessor)])
    DenoiseEngine.set_ip_scale(eng, [0.0, 0.4, 1.7])
    assert procs["a"].scale == procs["b"].scale == (0.0, 0.4, 1.7, 0.0, 0.4, 1.7)
    DenoiseEngine.set_ip_scale(eng, 0.4)
    assert procs["a"].scale == 0.4 and procs["b"].scale == 0.4
    with pytest.raises(ValueError, match="n_img = 3"):
        DenoiseEngine.set_ip_scale(eng, [0.0, 0.4])
    assert procs["a"].scale == 0.4


def test_generate_characters_refusals(tmp_path, monkeypatch):
    import numpy as np
    from PIL import Image
    from theatergen_amd import pipelines
    monkeypatch.chdir(tmp_path)
    Image.fromarray(np.full((8, 8, 3), 90, np.uint8)).save("model.png")
    db = str(tmp_path) + "/db_"
    Image.fromarray(np.full((8, 8, 3), 30, np.uint8)).save(db + "3.png")
    touched = []
    monkeypatch.setattr(pipelines, "_own_unet", lambda adapter, what: touched.append("unet") or types.SimpleNamespace())
    monkeypatch.setattr(pipelines, "_text_and_image_rows", lambda *a: (_ for _ in ()).throw(AssertionError("encoding started before the refusal")))
    lat = torch.zeros(2, 4, 16, 16)
    with pytest.raises(NotImplementedError, match="SDXL"):
        pipelines.generate_characters("story", [1, 2], "xl", ["a", "b"], db, None, lat, 4, [3, 7])
    with pytest.raises(ValueError, match="obj_id 7"):
        pipelines.generate_characters("story", [1, 2], "1.5", ["a fox", "a fox again"], db, None, lat, 4, [7, 7])
    with pytest.raises(ValueError, match="one entry per character"):
        pipelines.generate_characters("story", [1], "1.5", ["a", "b"], db, None, lat, 4, [3, 7])
    assert not os.path.exists(db + "7.png")
    # a duplicated obj_id that HAS its PNG is the reference's ordinary reuse: it gets past the refusals (and reaches the stubbed encoder)
    with pytest.raises(AssertionError, match="encoding started"):
        pipelines.generate_characters("story", [1, 2], "1.5", ["a", "b"], db, None, lat, 4, [3, 3])


def test_story_jobs_mark_first_appearances():
    from theatergen_amd import story
    jobs = story.story_jobs(0)
    assert story.job_ip_scales(jobs) == [0.4] * 8 and jobs == [story.CharacterJob(0, t, c) for t in range(1, 5) for c in range(2)]
    first = story.story_jobs(0, ip_scales="first")
    assert story.job_ip_scales(first) == [0.0, 0.0] + [0.4] * 6
    assert [(j.dialogue, j.turn, j.char, j.text_seed) for j in first] == [(j.dialogue, j.turn, j.char, j.text_seed) for j in jobs]
    assert story.job_ip_scales(story.story_jobs(1, turns=1, ip_scales=[0, 0.4])) == [0.0, 0.4]
    with pytest.raises(ValueError):
        story.story_jobs(0, ip_scales=[0.4])
