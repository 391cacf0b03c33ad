"""The streaming forms of the CRFP_simple / CRFP wirings without a GPU: the reference's MRCF_simple_v13 / MRCF_simple_v15 (model/CRFP_test.py:
1184-1486, 1805-2113; test_video.py's model codes 13 / 15) resolve under the ``MRCF_test`` name with the rig's constructor arguments, their
state_dict key / shape tables equal the reference's own (tests/golden/stream_ablation, make_stream_ablation_golden.py), and the C-ABI declares
and binds the four streaming entry points."""
import ast
import os
import re

import pytest
import torch

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("crfp_simple_stream_batch", "crfp_dense_stream_batch", "crfp_simple_stream_batch_bf16", "crfp_dense_stream_batch_bf16")


@pytest.fixture(scope="module")
def golden():
    return golden_io.load("stream_ablation")


@pytest.mark.parametrize("cls", ["MRCF_simple_v13", "MRCF_simple_v15"])
def test_test_video_builds_the_stream_classes(tmp_path, cls):
    """test_video.py:181,184: ``MRCF.MRCF_simple_v1x(mid_channels=32, y_only=, hr_dcn=, offset_prop=, spynet_pretrained='<fnet.pth>', device=)``."""
    from crfp_amd.model import CRFP, MRCF_test
    fnet = tmp_path / "fnet.pth"
    torch.save(CRFP.FNet(3).state_dict(), str(fnet))
    for hr_dcn, offset_prop in ((True, True), (False, True), (True, False)):
        m = getattr(MRCF_test, cls)(mid_channels=32, y_only=False, hr_dcn=hr_dcn, offset_prop=offset_prop, spynet_pretrained=str(fnet),
                                    device=torch.device("cpu"))
        assert callable(m.clear_states)
        m.clear_states()
        assert m.has_engine() == (hr_dcn and offset_prop)
    assert isinstance(m, CRFP.CRFP if cls.endswith("15") else CRFP.CRFP_simple)
    assert m._engine_class.__name__ == ("DenseStreamEngine" if cls.endswith("15") else "SimpleStreamEngine")


def test_state_dict_tables_equal_the_reference(golden):
    from crfp_amd.model import CRFP
    for name in golden["cases"]:
        name = str(name)
        kw = dict(ast.literal_eval(str(golden[f"{name}.kwargs"])))
        m = getattr(CRFP, str(golden[f"{name}.class"]))(device=torch.device("cpu"), **kw)
        got = [f"{k}:{','.join(map(str, v.shape))}" for k, v in m.state_dict().items()]
        assert got == [str(s) for s in golden[f"{name}.keys"]], name


def test_stream_classes_share_the_clip_models_table(golden):
    """The reference's stream classes hold exactly CRFP_simple's / CRFP's parameters (same keys, same shapes, same order)."""
    from crfp_amd.model import CRFP
    for stream, clip in (("MRCF_simple_v13", CRFP.CRFP_simple), ("MRCF_simple_v15", CRFP.CRFP)):
        for kw in (dict(mid_channels=32), dict(mid_channels=16, y_only=True, hr_dcn=False)):
            a = getattr(CRFP, stream)(device=torch.device("cpu"), **kw).state_dict()
            b = clip(device=torch.device("cpu"), **kw).state_dict()
            assert [(k, tuple(v.shape)) for k, v in a.items()] == [(k, tuple(v.shape)) for k, v in b.items()]


def test_golden_cases_cover_the_issue(golden):
    names = [str(n) for n in golden["cases"]]
    assert {"v13_mid32", "v15_mid32", "v15_yonly", "v13_nohrdcn", "v15_noprop"} <= set(names)
    for name in ("v13_mid32", "v15_mid32"):
        calls = golden[f"{name}.calls"]
        assert int(golden[f"{name}.t"]) == 7 and int(calls[-1][1]) == 7
        assert (calls[:, 1] - calls[:, 0] == 2).any() and int(golden[f"{name}.clear_at"]) > 0
        assert golden[f"{name}.fgs"].any() and not golden[f"{name}.fgs"].all()


def test_header_declares_and_bindings_cover_the_stream_entry_points():
    with open(os.path.join(ROOT, "include", "crfp_hip.h")) as f:
        hdr = f.read()
    from crfp_amd import _lib
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(const void\* packed, int flags, const float\* lr, const float\* lr_prev", hdr), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES["crfp_dsv_stream_batch"], name


def test_stream_engines_keep_the_clip_engines_refusals():
    """The clip handles keep refusing stream_frame; the stream handles bring DSVEngine's back and drive their wiring's own symbol."""
    from crfp_amd import engine
    assert engine.SimpleStreamEngine.stream_frame is engine.DSVEngine.stream_frame
    assert engine.DenseStreamEngine.clear_states is engine.DSVEngine.clear_states
    assert engine.SimpleEngine.stream_frame is engine.CRAEngine.stream_frame is engine.DenseEngine.stream_frame
    assert issubclass(engine.SimpleStreamEngine, engine.SimpleEngine) and issubclass(engine.DenseStreamEngine, engine.DenseEngine)
    e = object.__new__(engine.DenseStreamEngine)
    e.storage = "bf16"
    with pytest.raises(NotImplementedError):
        e._call("fnet_forward")
    # the workspace fetch reads the wiring's own Layout through the wiring's own symbol
    from crfp_amd import _lib
    assert _lib.symbol("dense", "debug_fetch", "bf16") == "crfp_dense_debug_fetch_bf16" and _lib.symbol("simple", "debug_fetch") == "crfp_simple_debug_fetch"
    assert engine.DenseStreamEngine.debug_fetch is engine.DSVEngine.debug_fetch

