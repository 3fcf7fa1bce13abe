"""The C ABI: every function declared in include/ngp_hip.h is exported by libngp_hip.so and bound by the ctypes layer with the
argument and return types of its prototype, and the package enters the library through _lib.call alone.  No compute calls: runs
without a GPU."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_hip.h")


def declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"NGP_API\s+[\w\s\*]+?\b(ngp_\w+)\s*\(", text)))


def prototypes():
    """name -> (return type, [parameter type, ...]) of every NGP_API prototype, types as the header spells them (no parameter names)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"NGP_API\s+([\w\s\*]+?)\b(ngp_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else [p if p.endswith("*") else re.sub(r"\s*\b\w+$", "", p) for p in params])
    return out


_C_SCALARS = {"int": ("int", 4), "int32_t": ("int", 4), "int64_t": ("int", 8), "uint32_t": ("uint", 4), "uint64_t": ("uint", 8), "size_t": ("uint", 8),
              "float": ("float", 4), "double": ("float", 8)}


def header_kind(ctype):
    """(class, bytes, is the stream) of a C parameter or return type"""
    if ctype == "ngp_stream_t":
        return "pointer", 8, True
    if "*" in ctype:
        return "pointer", 8, False
    return _C_SCALARS[ctype] + (False,)         # KeyError: a type this test does not know yet -- teach it, do not skip it


def ctypes_kind(t, stream_type):
    """the same triple of a ctypes type, by kind and ctypes.sizeof (c_int is c_int32 and c_size_t is c_uint64 here: class identity says nothing)"""
    if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)):
        assert ctypes.sizeof(t) == 8
        return "pointer", 8, issubclass(t, stream_type)
    assert issubclass(t, ctypes._SimpleCData), t
    code = t._type_
    kind = "float" if code in "fd" else "int" if code in "bhilq" else "uint" if code in "BHILQ" else None
    assert kind is not None, t
    return kind, ctypes.sizeof(t), False


def table_mismatches(signatures, restypes, stream_type):
    """every disagreement between the header's prototypes and a signature table, as text"""
    wrong = []
    for name, (ret, params) in prototypes().items():
        if name not in signatures:
            wrong.append(f"{name}: no entry")
            continue
        argtypes = signatures[name]
        if len(argtypes) != len(params):
            wrong.append(f"{name}: {len(params)} parameters in the header, {len(argtypes)} in the table")
            continue
        for i, (c, t) in enumerate(zip(params, argtypes)):
            if header_kind(c) != ctypes_kind(t, stream_type):
                wrong.append(f"{name}: parameter {i} is `{c}` {header_kind(c)} in the header, {t.__name__} {ctypes_kind(t, stream_type)} in the table")
        if header_kind(ret)[:2] != ctypes_kind(restypes.get(name, ctypes.c_int), stream_type)[:2] or (ret == "const char*") != (restypes.get(name) is ctypes.c_char_p):
            wrong.append(f"{name}: returns `{ret}` in the header, {restypes.get(name, ctypes.c_int).__name__} in the table")
    return wrong


def test_header_declares_the_four_reference_modules():
    names = declared()
    # raymarching/src/bindings.cpp:5-18, gridencoder/src/bindings.cpp:5-8, shencoder/src/bindings.cpp:5-8, ffmlp/src/bindings.cpp:5-11
    for ref_fn in ["near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "packbits", "march_rays_train",
                   "composite_rays_train_forward", "composite_rays_train_backward", "march_rays", "composite_rays", "grid_encode_forward",
                   "grid_encode_backward", "sh_encode_forward", "sh_encode_backward", "ffmlp_forward", "ffmlp_inference", "ffmlp_backward"]:
        assert f"ngp_{ref_fn}" in names
    assert "ngp_ffmlp_allocate_splitk" in names and "ngp_ffmlp_free_splitk" in names
    assert "ngp_render_rays" in names and "ngp_get_rays" in names


def test_library_exports_every_declared_symbol():
    from nerfsafetyvalidation_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "libngp_hip.so has not been built (python -c 'import __graft_entry__ as g; g.build()')"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)
    exported = set(re.findall(r" T (ngp_\w+)", out))
    missing = [n for n in declared() if n not in exported]
    assert not missing, f"declared in the header but not exported: {missing}"
    extra = [n for n in exported if n not in declared()]
    assert not extra, f"exported but not declared in include/ngp_hip.h: {extra}"


def test_ctypes_layer_binds_every_symbol():
    from nerfsafetyvalidation_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared()
    lib = _lib.lib()          # loading resolves every name and would raise AttributeError otherwise
    assert lib.ngp_version() >= 100
    assert isinstance(lib.ngp_last_error(), bytes)
    assert lib.ngp_march_rays_train_workspace(1000) >= 4000
    # caller-owned scratch sizes are host arithmetic (no GPU): split-K partials of the FFMLP weight gradients, bins of the grid scatter
    P = 64 * (32 + 64 + 16)
    # (one partial per workgroup of the fused backward: four per CU for this two-layer shape, 1024 -- more than the split-K plan's 1000)
    assert lib.ngp_ffmlp_backward_workspace(256 * 1000, 32, 64, 2) == 1024 * P * 4
    assert lib.ngp_ffmlp_backward_workspace(16, 32, 64, 2) == P * 4
    assert lib.ngp_grid_encode_backward_workspace(1 << 20, 3, 2, 16, _lib.NGP_F16) > 0
    assert lib.ngp_grid_encode_backward_workspace(1 << 20, 3, 2, 16, _lib.NGP_F32) == 0
    assert lib.ngp_grid_encode_backward_workspace(4096, 3, 2, 16, _lib.NGP_F16) == 0
    assert lib.ngp_packed_weights_bytes() == 4 * ((2048 + 2 * 4096 + 1024) + (2048 + 3 * 4096 + 1024))    # sized for the fp32 form
    assert ctypes.sizeof(_lib.ModelStruct) == 128 and ctypes.sizeof(_lib.RenderStats) == 40
    # LDS budget of the fused backward of `run` (host arithmetic): nerf/network.py's shapes in fp32 fit 512 samples per ray
    m = _lib.ModelStruct()
    m.sigma_hidden_mm, m.color_hidden_mm, m.precision = 0, 1, _lib.NGP_PREC_F32
    assert 0 < lib.ngp_render_uniform_backward_lds(ctypes.byref(m), 512) <= 160 * 1024
    m.sigma_hidden_mm, m.color_hidden_mm, m.precision = 1, 2, _lib.NGP_PREC_F16
    assert 0 < lib.ngp_render_uniform_backward_lds(ctypes.byref(m), 512) <= 160 * 1024


def test_backward_plans_answer_as_before_the_refactor(monkeypatch):
    """The workspace, buffer and recompute answers of the grid encoder's and the FFMLP's backward (host arithmetic, no GPU) over the
    sweep of tests/golden/make_golden_plans.py equal, value by value, those recorded from the build that preceded the shared
    backward plans (tests/golden/backward_plans.json), and the spot values worked out by hand there."""
    import importlib.util
    import json
    from nerfsafetyvalidation_amd import _lib
    for name in ("NGP_GRID_MERGE_MIN", "NGP_GRID_BIN_FILL_PCT"):
        monkeypatch.delenv(name, raising=False)
    spec = importlib.util.spec_from_file_location("make_golden_plans", os.path.join(ROOT, "tests", "golden", "make_golden_plans.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(gen.OUT))
    assert want["grid_axes"] == gen.GRID and want["ffmlp_axes"] == gen.FFMLP
    lib = _lib.lib()
    got = gen.answers(lib, _lib)
    assert len(got["grid_workspace"]) == 8 * 2 * 4 * 4 * 2 and len(got["ffmlp_workspace_buffer_recomputes"]) == 7 * 5 * 5 * 4
    for key, axes in (("grid_workspace", gen.GRID), ("ffmlp_workspace_buffer_recomputes", gen.FFMLP)):
        assert len(got[key]) == len(want[key])
        wrong = [(shape, g, w) for shape, g, w in zip(gen.sweep(axes), got[key], want[key]) if g != w]
        assert not wrong, f"{key}: {len(wrong)} shapes answer differently, first (shape, got, recorded): {wrong[:5]}"
    P = 64 * (32 + 64 + 16)
    assert P == 7168
    for B, partials in ((16, 1), (64, 1), (128, 2), (4096, 64), (1 << 20, 1024)):
        assert lib.ngp_ffmlp_backward_workspace(B, 32, 64, 2) == partials * P * 4
    for B, nbytes in ((131071, 0), (131072, 276824064), (1 << 25, 3225944064)):
        assert lib.ngp_grid_encode_backward_workspace(B, 3, 2, 16, _lib.NGP_F16) == nbytes


def test_workspace_sizes_answer_as_before_the_layouts():
    """Every size function whose entry point carves through csrc/workspace.hpp answers (host arithmetic, no GPU), over the sweep of
    tests/golden/make_golden_workspaces.py, what the build before the shared layouts answered (tests/golden/workspace_sizes.json) --
    except the density grid for H < 8, where the layout counts the partial sums the kernels write: there the answer is the listed new
    value, and no smaller than the bytes ngp_density_grid_update and ngp_density_grid_finish touch.  The size function that is new
    with the layouts, ngp_mark_untrained_grid_workspace, is checked against its definition."""
    import importlib.util
    import json
    from nerfsafetyvalidation_amd import _lib
    spec = importlib.util.spec_from_file_location("make_golden_workspaces", os.path.join(ROOT, "tests", "golden", "make_golden_workspaces.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    doc = json.load(open(gen.OUT))
    assert doc["cases"] == gen.CASES and sorted(doc["answers"]) == sorted(gen.CASES)
    lib = _lib.lib()
    got = gen.answers(lib)
    excepted = {(e["cascade"], e["H"]): e for e in gen.DENSITY_GRID_EXCEPTIONS}
    assert sorted(excepted) == [(c, H) for c in range(2, 9) for H in (2, 4)]
    wrong = []
    for name, shapes in gen.CASES.items():
        assert len(got[name]) == len(doc["answers"][name]) == len(shapes)
        for shape, g, w in zip(shapes, got[name], doc["answers"][name]):
            e = excepted.get(tuple(shape)) if name == "density_grid" else None
            if e is not None:
                c, H = shape
                assert w == e["old"] and e["new"] != e["old"], (shape, w, e)
                touched = H ** 3 * 8 + c * -(-H ** 3 // 256) * 8
                if g != e["new"] or g < touched:
                    wrong.append((name, shape, g, e["new"], touched))
            elif g != w:
                wrong.append((name, shape, g, w))
    assert not wrong, f"{len(wrong)} shapes answer differently, first (function, shape, got, recorded): {wrong[:5]}"
    # spot values by hand: the refusals answer 0, the thresholds sit where the header says
    assert lib.ngp_photo_loss_workspace(16384) == 0 and lib.ngp_photo_loss_workspace(16385) == 257 * 4
    assert lib.ngp_render_upsample_workspace(65535, 4, 2) == 0 and lib.ngp_render_upsample_workspace(65536, 4, 2) == 65536 * (8 * 4 + 6 * 32)
    assert lib.ngp_isosurface_workspace(2048, 1024, 1024) == 0 and lib.ngp_label_components_workspace(0, 5, 6) == 0
    assert lib.ngp_density_grid_workspace(8, 2) == 64 + 64 + 64 and lib.ngp_density_grid_workspace(1, 128) == (128 ** 3 + 128 ** 3 // 256) * 8 + 64
    # ngp_mark_untrained_grid_workspace: nothing up to 2048 cameras (one launch), a word per cell above, 0 for a grid the call refuses
    for n_cams, cascade, H, want in ((0, 1, 128, 0), (1, 3, 32, 0), (2048, 8, 128, 0), (2049, 3, 32, 3 * 32 ** 3 * 4), (5000, 8, 128, 8 * 128 ** 3 * 4),
                                     (2049, 1, 2, 32), (2049, 0, 32, 0), (2049, 9, 32, 0), (2049, 3, 48, 0), (2049, 1, 2048, 0)):
        assert lib.ngp_mark_untrained_grid_workspace(n_cams, cascade, H) == want, (n_cams, cascade, H)


def test_signature_table_matches_the_header():
    """Every prototype against its SIGNATURES / _RESTYPES entry: the number of parameters, per parameter the class (pointer, signed or
    unsigned integer, floating point) and the width, the return type (int, size_t, const char*), and the slot the table marks as the
    stream is the one the header declares ngp_stream_t.  A table with one argument dropped or one uint32 widened is caught."""
    from nerfsafetyvalidation_amd import _lib
    protos = prototypes()
    assert sorted(protos) == declared() == sorted(_lib.SIGNATURES)
    assert {r for r, _ in protos.values()} == {"int", "size_t", "const char*"}
    assert not set(_lib._RESTYPES) - set(_lib.SIGNATURES)
    wrong = table_mismatches(_lib.SIGNATURES, _lib._RESTYPES, _lib.StreamPtr)
    assert not wrong, "\n".join(wrong)
    # the stream: the last parameter wherever there is one, as _lib.call relies on
    with_stream = [n for n, (_, params) in protos.items() if "ngp_stream_t" in params]
    assert len(with_stream) > 80 and all(protos[n][1].index("ngp_stream_t") == len(protos[n][1]) - 1 for n in with_stream)
    # the check itself: it sees a dropped argument, a widened integer, a stream mark in the wrong place and a wrong return type
    broken = dict(_lib.SIGNATURES)
    broken["ngp_packbits"] = broken["ngp_packbits"][:-2] + broken["ngp_packbits"][-1:]
    broken["ngp_morton3D"] = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, _lib.StreamPtr]
    broken["ngp_sph_from_ray"] = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint32, _lib.StreamPtr, ctypes.c_void_p]
    found = table_mismatches(broken, {**_lib._RESTYPES, "ngp_version": ctypes.c_size_t}, _lib.StreamPtr)
    assert sorted(f.split(":")[0] for f in found) == ["ngp_morton3D", "ngp_packbits", "ngp_sph_from_ray", "ngp_sph_from_ray", "ngp_version"], found


def test_abi_version_is_one_number():
    from nerfsafetyvalidation_amd import _lib
    (in_header,) = re.findall(r"^#define NGP_ABI_VERSION (\d+)$", open(HEADER).read(), flags=re.M)
    assert int(in_header) == _lib.ABI_VERSION == _lib.lib().ngp_version()


def test_call_raises_with_the_name_the_code_and_the_library_message():
    import pytest
    import torch
    from nerfsafetyvalidation_amd import _lib
    with pytest.raises(RuntimeError) as err:
        _lib.call("debug_disable_march_queue", 1 << 4)
    text = str(err.value)
    assert "debug_disable_march_queue" in text and "code -1" in text and "unknown debug flag bits" in text
    assert _lib.call("debug_disable_march_queue", 0) is None
    # a host tensor is refused before the library is entered (the function's name is resolved first: a wrong name is an AttributeError)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.call("morton3D", torch.zeros(3, dtype=torch.int32), 1, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(AttributeError):
        _lib.call("no_such_function")
    with pytest.raises(TypeError, match="takes no stream"):
        _lib.call("debug_disable_march_queue", 0, stream=0)
    with pytest.raises(TypeError, match="ngp_morton3D takes 3 arguments and the stream; 4 given"):      # (a stream passed by hand, as before)
        _lib.call("morton3D", None, 0, None, 0)


def test_package_enters_the_library_through_call_alone():
    """_lib.check( -- the hand-written protocol -- occurs in the package only inside _lib.py"""
    pkg = os.path.join(ROOT, "nerfsafetyvalidation_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            path = os.path.join(dirpath, fn)
            if fn.endswith(".py") and path != os.path.join(pkg, "_lib.py"):
                assert "_lib.check(" not in open(path).read(), path


def test_product_never_imports_the_oracle():
    """only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/"""
    pkg = os.path.join(ROOT, "nerfsafetyvalidation_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".h", ".cpp")) or fn == "Makefile":
                text = open(os.path.join(dirpath, fn)).read()
                assert "import oracle" not in text and "from oracle" not in text and "ngp_oracle" not in text, os.path.join(dirpath, fn)


def test_cell_table_size_is_host_arithmetic():
    """ngp_cell_tables_bytes (no GPU work): 32 bytes per grid cell of the first n levels, with the level resolutions of
    gridencoder.cu:126-127 -- checked against the oracle's level geometry for the bound-2 Stonehenge table."""
    import numpy as np
    from nerfsafetyvalidation_amd import _lib
    from oracle import oracle as O
    import helpers as Hh
    offsets, pls = Hh.grid_offsets(input_dim=3, num_levels=16, log2_hashmap_size=19, desired_resolution=4096)
    S = float(np.log2(pls))
    m = _lib.ModelStruct()
    host = (ctypes.c_int32 * 17)(*[int(v) for v in offsets])
    m.offsets_host = ctypes.cast(host, ctypes.c_void_p)
    m.L, m.S, m.H_base, m.gridtype, m.align_corners = 16, S, 16, 0, 0
    lib = _lib.lib()
    res = [O.level_geometry(l, np.float32(S), 16)[1] for l in range(16)]
    for n in (4, 8, 12):
        assert lib.ngp_cell_tables_bytes(ctypes.byref(m), n) == 32 * sum(int(r) ** 3 for r in res[:n])
    assert lib.ngp_cell_tables_bytes(ctypes.byref(m), 16) == 0          # 4068^3 cells do not fit 32-bit record indices
    assert 38e9 < lib.ngp_cell_tables_bytes(ctypes.byref(m), 12) < 39e9


def test_library_reads_exactly_the_documented_switches():
    """The whole NUL-terminated strings of libngp_hip.so that look like a switch (NGP_[A-Z0-9_]+: the names it hands to getenv) are the
    rows of INTEGRATION.md's "Environment switches" table that the library reads -- no undocumented switch, no stale row."""
    from nerfsafetyvalidation_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    in_library = {s.decode() for s in blob.split(b"\0") if re.fullmatch(rb"NGP_[A-Z0-9_]+", s)}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("## Environment switches"):]
    table = table[:table.index("\n### ")]
    documented = set(re.findall(r"^\| `(NGP_[A-Z0-9_]+)` \| library \|", table, flags=re.M))
    assert len(documented) == 6
    assert in_library == documented


def test_debug_flag_names_and_validation():
    """_lib's NGP_DBG_* constants are the header's enum, and the process-default setter refuses a word with any other bit (host only)."""
    from nerfsafetyvalidation_amd import _lib
    enum = {n: 1 << int(b) for n, b in re.findall(r"(NGP_DBG_[A-Z_]+) = 1 << (\d+),", open(HEADER).read())}
    assert len(enum) == 11 and all(getattr(_lib, n) == v for n, v in enum.items())
    lib, every = _lib.lib(), sum(enum.values())
    try:
        assert lib.ngp_debug_disable_march_queue(every) == 0
        for bad in (1 << 4, 1 << 7, 1 << 9, 1 << 12, 1 << 19, every + (1 << 5), -1):
            assert lib.ngp_debug_disable_march_queue(bad) == -1, bad      # NGP_EINVAL
            assert b"unknown debug flag bits" in lib.ngp_last_error()
    finally:
        assert lib.ngp_debug_disable_march_queue(0) == 0
