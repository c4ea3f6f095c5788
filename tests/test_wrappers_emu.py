"""The helpers every stage wrapper is written with (DESIGN.md "Writing a stage wrapper"): _lib.call / _lib.scratch, the handle base
of instantsplat_amd/handles.py, BinningPolicy's capacity rule, _frames.frames_per_call — and the ctypes signature table of _lib
against include/mi355gs.h, type by type.  CPU tier: the emulated library where one is needed at all."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ _lib.call
def test_call_raises_naming_the_entry_point_and_the_code(emu):
    from instantsplat_amd import _lib
    src, dst = torch.zeros(3, 4, 4), torch.zeros(4, 4, 3, dtype=torch.uint8)
    _lib.call(emu, "rgb8_from_planar", _lib.STREAM, 4, 4, src, dst)   # accepted: no exception
    with pytest.raises(RuntimeError, match=r"^mi355gs: rgb8_from_planar failed: .+ \(-\d+\)$"):
        _lib.call(emu, "rgb8_from_planar", _lib.STREAM, 0, 4, src, dst)   # H = 0: EINVAL


def _record(monkeypatch, name):
    from instantsplat_amd import _lib
    seen = []
    monkeypatch.setattr(_lib.lib(), name, lambda *a: seen.append(a) or 0)
    return seen


def test_call_passes_tensors_as_addresses_none_as_null_and_the_rest_as_it_is(emu, monkeypatch):
    from instantsplat_amd import _lib
    seen = _record(monkeypatch, "mi355gs_rgb8_from_planar")
    t, table = torch.zeros(5), (ctypes.c_int32 * 2)(1, 2)
    _lib.call(emu, "rgb8_from_planar", 7, t, None, 0.5, t[2:], table, t.data_ptr() + 4)
    assert seen == [(7, t.data_ptr(), None, 0.5, t.data_ptr() + 8, table, t.data_ptr() + 4)]
    assert seen[0][5] is table


@pytest.mark.parametrize("position", [0, 1, 3])
def test_call_puts_the_stream_where_the_sentinel_stands(emu, monkeypatch, position):
    from instantsplat_amd import _lib
    seen = _record(monkeypatch, "mi355gs_rgb8_from_planar")
    asked = []
    monkeypatch.setattr(_lib, "stream_ptr", lambda dev: asked.append(dev) or 0x5EED)
    args = [11, 12, 13]
    args.insert(position, _lib.STREAM)
    _lib.call(emu, "rgb8_from_planar", *args)
    want = [11, 12, 13]
    want.insert(position, 0x5EED)
    assert seen == [tuple(want)] and asked == [emu]


# --------------------------------------------------------------------------------------------------------- _lib.scratch
def test_scratch_refuses_in_the_callers_words_and_returns_the_queried_bytes(emu):
    from instantsplat_amd import _lib
    with pytest.raises(ValueError, match=r"^no frames of 0 x 0 here$"):
        _lib.scratch(emu, "png_rgb8_scratch_bytes", 1, 0, 0, 0, what="no frames of 0 x 0 here")
    want = int(_lib.lib().mi355gs_png_rgb8_scratch_bytes(2, 9, 7, 0))
    got = _lib.scratch(emu, "png_rgb8_scratch_bytes", 2, 9, 7, 0, what="unused")
    assert want > 0 and got.dtype == torch.uint8 and got.device == emu and tuple(got.shape) == (want,)
    assert _lib.scratch(emu, "png_rgb8_scratch_bytes", 1, 0, 0, 0, what=None).numel() == 1   # what=None: nothing is refused


# ------------------------------------------------------------------------------------------------------ frames_per_call
def _fits(limit, log=None):
    def fits(n):
        if log is not None:
            log.append(n)
        return n <= limit
    return fits


@pytest.mark.parametrize("limit, cap, estimate, want", [
    (0, 100, 0, 1),            # a budget below one frame: one frame per call all the same
    (0, 100, 50, 1),
    (37, 100, 37, 37),         # the estimate exactly right
    (37, 100, 38, 37),         # one too high (the buffers' padding)
    (10 ** 9, 500, 3, 500),    # far too low: grows to cap
    (10 ** 9, 1, 7, 1),        # cap = 1
    (0, 1, 0, 1),
    (10 ** 9, 65535, 65535, 65535),   # everything fits at the largest call the library takes
    (10 ** 9, 65535, 10 ** 12, 65535),
])
def test_frames_per_call(limit, cap, estimate, want):
    from instantsplat_amd._frames import frames_per_call
    log = []
    assert frames_per_call(_fits(limit, log), cap, estimate) == want
    assert all(1 <= n <= cap for n in log) and len(log) <= abs(min(cap, max(estimate, 1)) - want) + 2


# ----------------------------------------------------------------------------------------------------------- the handles
def _gaussians(P=5, rest=15, **over):
    g = dict(_xyz=torch.zeros(P, 3), _features_dc=torch.zeros(P, 1, 3), _features_rest=torch.zeros(P, rest, 3), _opacity=torch.zeros(P, 1),
             _scaling=torch.zeros(P, 3), _rotation=torch.zeros(P, 4))
    g.update(over)
    return types.SimpleNamespace(**g)


def _handle_classes():
    from instantsplat_amd.pose_tracking import FusedPoseTracker
    from instantsplat_amd.render_path import FusedPathRenderer
    return (FusedPoseTracker, "tracker", "fused pose tracking"), (FusedPathRenderer, "path", "path rendering")


def test_handle_close_twice_destroys_once_and_del_after_close_is_silent(emu, monkeypatch):
    from instantsplat_amd import _lib
    for cls, prefix, _ in _handle_classes():
        destroyed = []
        real = getattr(_lib.lib(), f"mi355gs_{prefix}_destroy")
        monkeypatch.setattr(_lib.lib(), f"mi355gs_{prefix}_destroy", lambda h, real=real, destroyed=destroyed: destroyed.append(h.value) or real(h))
        h = cls(_gaussians(), 16, 16, 64)
        value = h.handle
        assert value and h.workspace.numel() == int(getattr(_lib.lib(), f"mi355gs_{prefix}_workspace_bytes")(5, 16, 16, 64))
        assert h._h.value == value
        h.close()
        h.close()
        h.__del__()
        assert destroyed == [value] and h.handle is None


def test_handle_close_survives_a_library_that_is_gone(monkeypatch):
    from instantsplat_amd import _lib
    from instantsplat_amd.handles import LibraryHandle
    h = LibraryHandle()
    h.prefix, h.handle = "tracker", 1234
    monkeypatch.setattr(_lib, "lib", None)   # interpreter shutdown: module globals are cleared before the last objects die
    h.__del__()
    assert h.handle is None
    LibraryHandle.__new__(LibraryHandle).close()   # a constructor that raised before it had a handle


def test_handle_refuses_parameters_of_the_wrong_shape_or_dtype_in_its_own_words(emu, monkeypatch):
    from instantsplat_amd import _lib
    for cls, prefix, phrase in _handle_classes():
        monkeypatch.setattr(_lib.lib(), f"mi355gs_{prefix}_create", lambda *a: pytest.fail("create was called"))
        with pytest.raises(ValueError, match=phrase + r" needs float32 parameters of shape \(5, 3\)"):
            cls(_gaussians(_scaling=torch.zeros(5, 2)), 16, 16, 64)
        with pytest.raises(ValueError, match=phrase + r" needs float32 parameters of shape \(5, 1\), got \(5, 1\) torch.float64"):
            cls(_gaussians(_opacity=torch.zeros(5, 1, dtype=torch.float64)), 16, 16, 64)
        with pytest.raises(ValueError, match=phrase):
            cls(_gaussians(_features_rest=torch.zeros(4, 15, 3)), 16, 16, 64)


def test_handle_refuses_a_rejected_workspace_size_before_create(emu, monkeypatch):
    from instantsplat_amd import _lib
    for cls, prefix, _ in _handle_classes():
        created = []
        monkeypatch.setattr(_lib.lib(), f"mi355gs_{prefix}_create", lambda *a, created=created: created.append(a))
        for W, H, capacity in ((0, 16, 64), (16, 16, 0)):
            with pytest.raises(ValueError, match=f"mi355gs_{prefix}_workspace_bytes rejected the sizes"):
                cls(_gaussians(), W, H, capacity)
        assert created == []


# -------------------------------------------------------------------------------------------------------- BinningPolicy
@pytest.mark.parametrize("slack, pad", [(1.5, 16384), (0.5, 0), (1.0000001, 3)])
def test_capacity_rule_is_the_expression_it_replaced(monkeypatch, slack, pad):
    from instantsplat_amd.diff_gaussian_rasterization import BinningPolicy
    monkeypatch.setattr(BinningPolicy, "slack", slack)
    monkeypatch.setattr(BinningPolicy, "pad", pad)
    for count in (0, 1, 7, 2 ** 31 - 1):
        assert BinningPolicy.capacity_for(count) == int(BinningPolicy.slack * count) + BinningPolicy.pad
        assert isinstance(BinningPolicy.capacity_for(count), int)
        for capacity in (1, 10 ** 6):
            assert BinningPolicy.regrown(count, capacity) == max(int(BinningPolicy.slack * count) + BinningPolicy.pad, 2 * capacity)
    assert BinningPolicy.capacity_for(7) == int(slack * 7) + pad   # truncated, not rounded: 10 at the default slack


# ------------------------------------------------------------------------------------- _lib._SIGNATURES vs the header
_SCALARS = {"int": "c_int", "int32_t": "c_int", "int64_t": "c_int64", "size_t": "c_size_t", "float": "c_float", "uint32_t": "c_uint32"}


def _header_prototypes():
    """{name: (return type text, [parameter text])} of every mi355gs_* prototype of include/mi355gs.h"""
    src = open(os.path.join(ROOT, "include", "mi355gs.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    src = src.replace('extern "C" {', " ")
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(mi355gs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in protos, f"{name} is declared twice"
        protos[name] = (ret, [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    mentioned = set(re.findall(r"\b(mi355gs_[a-z0-9_]+)\s*\(", src))
    assert mentioned == set(protos), f"prototypes this test cannot parse: {sorted(mentioned ^ set(protos))}"
    return protos


def _is_pointer(ctype):
    return ctype is ctypes.c_void_p or (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))


def _mismatch(text, ctype, is_return):
    """None if the ctypes class fits the C declaration `text`, else what the declaration asks for"""
    text = re.sub(r"\blong\s+long\b", "int64_t", text)   # (the header spells a few 64-bit strides that way)
    words = [w for w in re.findall(r"[A-Za-z_]\w*", text) if w != "const"]
    if "*" in text or "[" in text:
        if is_return and words == ["char"]:
            return None if ctype is ctypes.c_char_p else "c_char_p"
        return None if _is_pointer(ctype) else "c_void_p or a POINTER(...)"
    if is_return and words == ["void"]:
        return None if ctype is None else "None"
    assert words and words[0] in _SCALARS and len(words) <= (1 if is_return else 2), f"a type this test does not know: {text!r}"
    return None if ctype is getattr(ctypes, _SCALARS[words[0]]) else _SCALARS[words[0]]


def test_signature_table_matches_the_header_type_by_type():
    """Every entry of _lib._SIGNATURES against its prototype: the return type and each parameter's class.  The library is not
    loaded.  (test_c_abi_library_exports_every_declared_symbol compares the NAMES; a c_int where the header says int64_t would
    pass it and corrupt an argument.)"""
    from instantsplat_amd import _lib
    protos = _header_prototypes()
    assert set(protos) == set(_lib._SIGNATURES), set(protos) ^ set(_lib._SIGNATURES)
    assert len(protos) >= 94
    wrong = []
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib._SIGNATURES[name]
        need = _mismatch(ret, restype, True)
        if need:
            wrong.append(f"{name}: returns `{ret}`, the table says {getattr(restype, '__name__', restype)}, not {need}")
        if len(params) != len(argtypes):
            wrong.append(f"{name}: {len(params)} parameters in the header, {len(argtypes)} in the table")
            continue
        for k, (text, ctype) in enumerate(zip(params, argtypes)):
            need = _mismatch(text, ctype, False)
            if need:
                wrong.append(f"{name}: parameter {k} is `{text}`, the table says {getattr(ctype, '__name__', ctype)}, not {need}")
    assert not wrong, "\n".join(wrong)


def test_signature_check_sees_a_wrong_width_and_a_prototype_it_cannot_parse():
    assert _mismatch("int64_t n", ctypes.c_int, False) == "c_int64" and _mismatch("int64_t n", ctypes.c_int64, False) is None
    assert _mismatch("const float* a", ctypes.c_int64, False) and _mismatch("const int channels[5]", ctypes.c_void_p, False) is None
    assert _mismatch("double* total_ms", ctypes.POINTER(ctypes.c_double), False) is None
    assert _mismatch("const char*", ctypes.c_char_p, True) is None and _mismatch("const char*", ctypes.c_void_p, True) == "c_char_p"
    assert _mismatch("void", None, True) is None and _mismatch("void", ctypes.c_int, True) == "None"
    assert _mismatch("size_t", ctypes.c_int64, True) == "c_size_t"
    with pytest.raises(AssertionError, match="does not know"):
        _mismatch("unsigned long n", ctypes.c_int64, False)
