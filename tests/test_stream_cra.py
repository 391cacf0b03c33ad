"""The streaming form of the CRFP_DSV_CRA wiring without a GPU: the reference's MRCF_simple_v18_cra (model/CRFP_test.py:2480-2861) resolves
under the ``MRCF_test`` name, its state_dict key / shape table equals the reference's own (tests/golden/stream_cra,
make_stream_cra_golden.py) and CRFP_DSV_CRA's, the wiring's row of the binding table carries ``stream_batch`` for both storage types, the
C-ABI declares and exports the two entry points, and the handles offer / refuse them as their classes say."""
import ast
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("crfp_cra_stream_batch", "crfp_cra_stream_batch_bf16")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def golden():
    return golden_io.load("stream_cra")


def _table(m):
    return [f"{k}:{','.join(map(str, v.shape))}" for k, v in m.state_dict().items()]


def _lib_row(key):
    from crfp_amd import _lib
    return _lib.FAMILIES[key]


def test_cra_row_carries_stream_batch_for_both_storages():
    from crfp_amd import _lib
    row = _lib.FAMILIES["cra"]
    assert "stream_batch" in row.ops and "stream_batch" in row.bf16
    assert row.ops == _lib.FAMILIES["simple"].ops and row.bf16 == _lib.FAMILIES["simple"].bf16   # nothing else in the row changed
    assert (row.prefix, row.names, row.num_params, row.model) == ("crfp_cra_", "cra", _lib.CRA_NUM_PARAMS, "CRFP_DSV_CRA")
    assert [_lib.symbol("cra", "stream_batch", st) for st in ("f32", "bf16")] == list(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES["crfp_dsv_stream_batch"], name


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "crfp_hip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    raw = ctypes.CDLL(so)
    dsv = re.search(r"\bint\s+crfp_dsv_stream_batch(\(.*?\));", hdr, flags=re.S).group(1)
    for name in NEW_SYMBOLS:
        got = re.search(r"\bint\s+" + name + r"(\(.*?\));", hdr, flags=re.S)
        assert got, f"{name} is not declared in include/crfp_hip.h"
        assert re.sub(r"\s+", " ", got.group(1)) == re.sub(r"\s+", " ", dsv), name     # exactly crfp_dsv_stream_batch's signature
        assert hasattr(raw, name), f"{name} declared in include/crfp_hip.h but not exported"


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_stream_handle_offers_what_the_clip_handle_withholds(storage):
    from crfp_amd import engine
    ops = ("param_numel", "packed_weight_bytes", "pack_weights", "batch_workspace_bytes", "batch_status_offset", "forward_batch", "stream_batch")
    s = object.__new__(engine.CRAStreamEngine)
    c = object.__new__(engine.CRAEngine)
    for e in (s, c):
        e.storage = storage
        e._fns = dict.fromkeys(ops, "bound")
    assert s._call("stream_batch") == "bound" and s.WIRING == c.WIRING == "cra"
    with pytest.raises(NotImplementedError, match="CRFP_DSV_CRA") as err:
        c._call("stream_batch")
    assert "CRAStreamEngine" in str(err.value)
    with pytest.raises(NotImplementedError):
        c.stream_frame(None, None, None)
    for e in (s, c):
        assert e._call("forward_batch") == "bound"
        with pytest.raises(NotImplementedError, match="CRFP_DSV_CRA"):
            e._call("fnet_forward")
        with pytest.raises(KeyError):      # debug_fetch is in the row (crfp_cra_debug_fetch); this hand-made table of bound functions lacks it
            e._call("debug_fetch")
        assert "debug_fetch" in _lib_row("cra").ops and type(e).debug_fetch is engine.DSVEngine.debug_fetch
    assert issubclass(engine.CRAStreamEngine, engine.CRAEngine) and engine.CRAStreamEngine._withheld == frozenset()
    assert engine.CRAStreamEngine.stream_frame is engine.DSVEngine.stream_frame
    assert engine.CRAStreamEngine.clear_states is engine.DSVEngine.clear_states
    # the clip handles of the ablation wirings still withhold it
    assert "stream_batch" in engine.SimpleEngine._withheld and "stream_batch" in engine.DenseEngine._withheld


def test_model_has_the_reference_table_and_the_clip_models(golden):
    from crfp_amd.model import CRFP, MRCF_test
    assert MRCF_test.MRCF_simple_v18_cra is CRFP.MRCF_simple_v18_cra
    m = CRFP.MRCF_simple_v18_cra(CPU, mid_channels=32)
    assert _table(m) == [str(s) for s in golden["cra_mid32.keys"]]
    assert _table(m) == _table(CRFP.CRFP_DSV_CRA(CPU, mid_channels=32))
    assert isinstance(m, CRFP.CRFP_DSV_CRA) and m._engine_class.__name__ == "CRAStreamEngine" and callable(m.clear_states)
    m.clear_states()
    for name in map(str, golden["cases"]):
        assert str(golden[f"{name}.class"]) == "MRCF_simple_v18_cra"
        kw = dict(ast.literal_eval(str(golden[f"{name}.kwargs"])))
        assert _table(CRFP.MRCF_simple_v18_cra(device=CPU, **kw)) == [str(s) for s in golden[f"{name}.keys"]], name
        assert _table(CRFP.CRFP_DSV_CRA(device=CPU, **kw)) == [str(s) for s in golden[f"{name}.keys"]], name


def test_constructor_arguments_and_engine_paths(tmp_path):
    """The reference's constructor (:2481); split_ratio other than 3 raises as in MRCF_simple_v18; the engine exists for mid_channels 32 and
    16 with both flags on, every other combination streams through the composition."""
    from crfp_amd.model import CRFP
    with pytest.raises(NotImplementedError):
        CRFP.MRCF_simple_v18_cra(CPU, split_ratio=2)
    fnet = tmp_path / "fnet.pth"
    torch.save(CRFP.FNet(3).state_dict(), str(fnet))
    for mid, hr_dcn, offset_prop, eng in ((32, True, True, True), (16, True, True, True), (64, True, True, False), (32, False, True, False),
                                          (32, True, False, False)):
        m = CRFP.MRCF_simple_v18_cra(device=CPU, mid_channels=mid, y_only=False, hr_dcn=hr_dcn, offset_prop=offset_prop, split_ratio=3,
                                     spynet_pretrained=str(fnet))
        assert m.has_engine() == eng, (mid, hr_dcn, offset_prop)
    d = CRFP.MRCF_simple_v18_cra(CPU)
    assert (d.mid_channels, d.y_only, d.hr_dcn, d.offset_prop, d.split_ratio) == (16, False, True, True, 3)
    assert (d.storage, d.precision, d.on_overflow, d.inputs_resident) == ("f32", "split", "poison", False)
    # the clip model keeps refusing the one-frame-per-call interface
    with pytest.raises(NotImplementedError):
        CRFP.CRFP_DSV_CRA(CPU).forward_stream(None, None, None)


def test_golden_cases_cover_the_issue(golden):
    sa = golden_io.load("stream_ablation")
    assert [str(n) for n in golden["cases"]] == ["cra_mid32", "cra_yonly", "cra_mid16"]
    assert all(int(golden[k]) == int(sa[k]) for k in ("h", "w", "fv"))        # stream_ablation's geometry and fovea size
    assert golden["cra_mid32.calls"].tolist() == [[0, 1], [1, 2], [2, 4], [4, 5], [5, 6], [6, 7]]
    assert int(golden["cra_mid32.t"]) == 7 and int(golden["cra_mid32.clear_at"]) == 3
    for name in ("cra_yonly", "cra_mid16"):
        assert int(golden[f"{name}.t"]) == 3 and golden[f"{name}.calls"].tolist() == [[0, 1], [1, 2], [2, 3]]
    assert str(golden["cra_mid16.kwargs"]) == "[]" and "y_only" in str(golden["cra_yonly.kwargs"])
    h, w = int(golden["h"]), int(golden["w"])
    for name, t, co in (("cra_mid32", 7, 3), ("cra_yonly", 3, 1), ("cra_mid16", 3, 3)):
        fgs = golden[f"{name}.fgs"]
        assert fgs.shape == (1, t, 1, 8 * h, 8 * w) and all(fgs[0, i].any() and not fgs[0, i].all() for i in range(t))   # a box per frame
        assert golden[f"{name}.out"].shape == (1, t, co, 8 * h, 8 * w) and np.isfinite(golden[f"{name}.out"]).all()


def test_committed_script_reproduces_the_golden_bit_for_bit(golden, tmp_path):
    sys.path.insert(0, golden_io.GOLDEN)
    try:
        import make_golden
    finally:
        sys.path.remove(golden_io.GOLDEN)
    if not os.path.isdir(make_golden.REF):
        pytest.skip("the reference is not mounted here")
    subprocess.check_call([sys.executable, os.path.join(golden_io.GOLDEN, "make_stream_cra_golden.py"), str(tmp_path)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    again = golden_io.load("stream_cra", str(tmp_path))
    assert sorted(again) == sorted(golden)
    for k, v in golden.items():
        assert again[k].dtype == v.dtype and again[k].shape == v.shape and again[k].tobytes() == v.tobytes(), k
