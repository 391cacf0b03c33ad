"""The wiring table ``crfp_amd._lib.FAMILIES`` without a GPU: every row resolves to bound, declared C names, every per-family binding is
reachable from a row, the handle classes refuse exactly what their wiring lacks, and the models' shared repack mixin adds nothing to a
state_dict."""
import ast
import os
import re

import pytest
import torch

import golden_io

from crfp_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the C-ABI's n = 1 conveniences (crfp_dsv_forward_clip = crfp_dsv_forward_batch with n = 1, and so on): exported and bound, used by no handle
N1_CONVENIENCES = {f"crfp_dsv_{n}{s}" for n in ("forward_clip", "stream_frame", "workspace_bytes", "status_offset") for s in ("", "_bf16")}
CLIP_REFUSED = {"stream_batch", "fnet_forward"}      # every wiring has a debug_fetch of its own Layout
REFUSED = {"DSVEngine": set(), "CRAEngine": CLIP_REFUSED, "SimpleEngine": CLIP_REFUSED, "DenseEngine": CLIP_REFUSED,
           "SimpleStreamEngine": CLIP_REFUSED - {"stream_batch"}, "DenseStreamEngine": CLIP_REFUSED - {"stream_batch"}}
DSV_OPS = {"param_numel", "packed_weight_bytes", "pack_weights", "batch_workspace_bytes", "batch_status_offset", "forward_batch",
           "stream_batch", "fnet_forward", "debug_fetch"}


def _declared():
    with open(os.path.join(ROOT, "include", "crfp_hip.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(crfp_[a-z0-9_]+)\s*\(", hdr))


def _reachable():
    names = set()
    for key, row in _lib.FAMILIES.items():
        names.add(_lib.FAMILIES[row.names].prefix + "param_name")
        names |= {_lib.symbol(key, op, st) for op in row.ops for st in ("f32", "bf16")}
    return names


def test_rows_name_the_five_families():
    assert list(_lib.FAMILIES) == ["dsv", "cra", "simple", "dense", "rt"]
    assert [r.prefix for r in _lib.FAMILIES.values()] == ["crfp_dsv_", "crfp_cra_", "crfp_simple_", "crfp_dense_", "crfp_rt_"]
    assert [r.model for r in _lib.FAMILIES.values()] == ["CRFP_DSV", "CRFP_DSV_CRA", "CRFP_simple", "CRFP", "MRCF_simple_v18"]
    assert [r.names for r in _lib.FAMILIES.values()] == ["dsv", "cra", "dsv", "dsv", "rt"]
    assert [r.num_params for r in _lib.FAMILIES.values()] == [_lib.NUM_PARAMS, _lib.CRA_NUM_PARAMS, _lib.NUM_PARAMS, _lib.NUM_PARAMS, _lib.RT_NUM_PARAMS]
    assert _lib.FAMILIES["dsv"].ops == DSV_OPS
    for key in ("cra", "simple", "dense"):      # everything CRFP_DSV has but the stand-alone flow network call, the fetch in both storage types
        assert _lib.FAMILIES[key].ops == DSV_OPS - {"fnet_forward"} and "debug_fetch" in _lib.FAMILIES[key].bf16
        assert _lib.symbol(key, "debug_fetch", "bf16") == f"crfp_{key}_debug_fetch_bf16"
        assert _lib.SIGNATURES[f"crfp_{key}_debug_fetch"] == _lib.SIGNATURES["crfp_dsv_debug_fetch"]
    assert _lib.FAMILIES["rt"].ops == {"param_numel", "packed_weight_bytes", "pack_weights", "workspace_bytes", "forward_clip", "debug_fetch"}
    # the regional fetch takes the seven-number geometry: an argument list of its own, not CRFP_DSV's
    assert _lib.SIGNATURES["crfp_rt_debug_fetch"] != _lib.SIGNATURES["crfp_dsv_debug_fetch"]
    assert len(_lib.SIGNATURES["crfp_rt_debug_fetch"][1]) == len(_lib.SIGNATURES["crfp_dsv_debug_fetch"][1]) + 4
    for row in _lib.FAMILIES.values():
        assert row.bf16 <= row.ops and "param_numel" not in row.bf16
    assert not _lib.FAMILIES["rt"].bf16


def test_every_operation_of_a_row_is_bound_and_declared():
    declared = _declared()
    for key, row in _lib.FAMILIES.items():
        for op in row.ops:
            for storage in ("f32", "bf16"):
                name = _lib.symbol(key, op, storage)
                assert name in _lib.SIGNATURES and name in declared, (key, op, storage, name)
                assert name.endswith("_bf16") == (storage == "bf16" and op in row.bf16), name
        for op in DSV_OPS - row.ops:
            with pytest.raises(NotImplementedError):
                _lib.symbol(key, op)


def test_every_family_binding_is_reachable_from_a_row():
    family = {n for n in _lib.SIGNATURES if re.match(r"crfp_(dsv|cra|simple|dense|rt)_", n)}
    assert N1_CONVENIENCES <= family
    assert family - _reachable() == N1_CONVENIENCES
    assert _reachable() - family == {"crfp_fnet_forward", "crfp_fnet_forward_bf16"}   # the flow network alone has no family prefix


@pytest.mark.parametrize("cls", sorted(REFUSED))
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_handles_refuse_exactly_what_their_wiring_lacks(cls, storage):
    """On a handle made without __init__: the refusal comes before the library, the arguments or the handle's state are looked at."""
    e = object.__new__(getattr(engine, cls))
    e.storage = storage
    e._fns = dict.fromkeys(DSV_OPS, "bound")       # what _bind() would have resolved
    assert e.MODEL_NAME == _lib.FAMILIES[e.WIRING].model
    for op in DSV_OPS:
        if op in REFUSED[cls]:
            with pytest.raises(NotImplementedError, match=e.MODEL_NAME):
                e._call(op)
        else:
            assert e._call(op) == "bound"
    for op, method, args in (("stream_batch", "stream_frame", (None, None, None)), ("fnet_forward", "compute_flow", (None, None)),
                             ("debug_fetch", "debug_fetch", (None, 1, 8, 8))):
        if op in REFUSED[cls]:
            with pytest.raises(NotImplementedError):
                getattr(e, method)(*args)


def test_runtime_handle_reads_its_row():
    e = object.__new__(engine.RuntimeEngine)
    assert (e.WIRING, e.MODEL_NAME, e.storage) == ("rt", "MRCF_simple_v18", "f32")
    with pytest.raises(NotImplementedError):
        e._call("forward_batch")
    e._fns = dict.fromkeys(_lib.FAMILIES["rt"].ops, "bound")
    for op in _lib.FAMILIES["rt"].ops:
        assert e._call(op) == "bound"
    assert _lib.symbol("rt", "debug_fetch") == _lib.symbol("rt", "debug_fetch", "bf16") == "crfp_rt_debug_fetch"
    with pytest.raises(RuntimeError, match="before any forward"):      # no forward yet: nothing is read, the library is not called
        e.debug_fetch("state")
    assert engine.RuntimeEngine.WEIGHT_LIMIT_SPLIT == engine.DSVEngine.WEIGHT_LIMIT_SPLIT == 32.0


def _table(m):
    return [f"{k}:{','.join(map(str, v.shape))}" for k, v in m.state_dict().items()]


def test_repack_mixin_leaves_every_state_dict_alone():
    from crfp_amd.model import CRFP, MRCF_runtime
    cpu = torch.device("cpu")
    simple, rt = CRFP.CRFP_simple(cpu, mid_channels=32), MRCF_runtime.MRCF_simple_v18(cpu, mid_channels=32)
    for m in (simple, rt, CRFP.CRFP_DSV(cpu), CRFP.MRCF_simple_v15(cpu)):
        assert isinstance(m, engine.PackedModel) and callable(m.invalidate_packed) and callable(m.engine)
        assert m._engine is None and m._engine_sig is None and not any(k.startswith("_engine") for k in m.state_dict())
        m.invalidate_packed()
    assert not isinstance(engine.PackedModel(), torch.nn.Module)
    assert [type(m)._engine_class.__name__ for m in (simple, CRFP.CRFP(cpu), CRFP.CRFP_DSV(cpu), CRFP.CRFP_DSV_CRA(cpu))] == \
        ["SimpleEngine", "DenseEngine", "DSVEngine", "CRAEngine"]
    # the tables the reference's own classes have: the goldens of tests/test_flags.py, test_stream_ablation.py and test_host_logic.py
    assert list(rt.state_dict()) == [str(k) for k in golden_io.load("runtime_small")["keys"]]
    by_prefix = {"cra": "CRFP_DSV_CRA", "simple": "CRFP_simple", "dense": "CRFP"}      # dsv_flags names its cases by wiring
    for gname in ("dsv_flags", "stream_ablation"):
        g = golden_io.load(gname)
        built = 0
        for name in map(str, g["cases"]):
            if f"{name}.ctor_error" in g:
                continue
            cls = str(g[f"{name}.class"]) if f"{name}.class" in g else by_prefix.get(name.split("_")[0], "CRFP_DSV")
            m = getattr(CRFP, cls)(device=cpu, **dict(ast.literal_eval(str(g[f"{name}.kwargs"]))))
            assert _table(m) == [str(s) for s in g[f"{name}.keys"]], (gname, name)
            built += 1
        assert built >= 5, gname
