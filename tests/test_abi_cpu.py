"""CPU suite: the C-ABI library loads without a GPU and exports every symbol include/crowdstep.h declares."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_and_exports_every_declared_symbol():
    import __graft_entry__ as g

    g.build()
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "crowdstep.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", header))
    declared -= {"cs_status"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"libcrowdstep.so does not export {name}"
    assert set(_lib.ABI_SYMBOLS) == declared
    assert lib.cs_abi_version() == _lib.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "crowdstep.h")).read()
    assert "#define CS_ABI_VERSION 4" in hdr          # header, library and binding name one ABI


# include/crowdstep.h type -> ctypes, as social_navigation_pyenvs_amd/_lib.py ABI states them; every pointer not named here is a c_void_p
_HEADER_TYPES = {"int": "c_int", "int32_t": "c_int", "unsigned": "c_uint", "uint32_t": "c_uint", "unsigned long long": "c_ulonglong",
                 "size_t": "c_size_t", "float": "c_float", "double": "c_double"}
_HEADER_STRUCTS = ("cs_worlds", "cs_worlds_f64", "cs_generator", "cs_gym_book", "cs_stage_book")
_HEADER_RESULTS = {"int": "c_int", "size_t": "c_size_t", "const char*": "c_char_p"}


def _header_prototypes(header):
    """{symbol: (restype, [argtypes])} of every prototype of the header; ValueError on a parameter type the mapping does not know."""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib

    out = {}
    for m in re.finditer(r"^(int|size_t|const char\*) (cs_\w+)\(([^;]*?)\);", header, re.M | re.S):
        res, name, params = m.groups()
        args = []
        for p in re.sub(r"/\*.*?\*/", " ", params, flags=re.S).split(","):
            p = " ".join(p.split())
            if p == "void":
                continue
            t = re.sub(r"\s*\*", "*", re.sub(r"\s*\b\w+$", "", p))     # without the parameter's name; "float *" -> "float*"
            if t in _HEADER_TYPES:
                args.append(getattr(C, _HEADER_TYPES[t]))
            elif t.startswith("const cs_") and t[6:-1] in _HEADER_STRUCTS and t.endswith("*") and t.count("*") == 1:
                args.append(C.POINTER(getattr(_lib, t[6:-1])))
            elif re.fullmatch(r"(const )?(void|char|int|float|double|size_t|u?int(8|32)_t|unsigned long long)\*( const\*|\*)?", t):
                args.append(C.c_void_p)
            else:
                raise ValueError(f"{name}: parameter type {t!r} ({p!r}) has no ctypes mapping")
        out[name] = (getattr(C, _HEADER_RESULTS[res]), args)
    return out


def test_signature_table_is_the_header():
    """Every prototype of include/crowdstep.h, parsed, is the (restype, argtypes) entry of _lib.ABI, and the loaded library's functions
    carry exactly those."""
    from social_navigation_pyenvs_amd import _lib

    header = open(os.path.join(ROOT, "include", "crowdstep.h")).read()
    protos = _header_prototypes(header)
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", header)) - {"cs_status"}
    assert set(protos) == declared == set(_lib.ABI)
    lib = _lib.load()
    for name, (restype, argtypes) in protos.items():
        assert (_lib.ABI[name][0], list(_lib.ABI[name][1])) == (restype, argtypes), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    with pytest.raises(ValueError, match="no ctypes mapping"):
        _header_prototypes("int cs_x(int a, long b);")
    with pytest.raises(ValueError, match="no ctypes mapping"):
        _header_prototypes("int cs_x(const cs_unknown* u);")


def test_wrong_arguments_are_refused_in_python_before_c():
    """A descriptor of the other precision, a float for an int, an int wrapper for a float, a short argument list: ctypes refuses each
    by the header's types, nothing reaches the library."""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    w32, w64 = _lib.cs_worlds(), _lib.cs_worlds_f64()
    refused = (C.ArgumentError, TypeError)
    with pytest.raises(refused):
        lib.cs_step(C.byref(w64), 0.0125, 1, None, None)
    with pytest.raises(refused):
        lib.cs_step_f64(C.byref(w32), 0.0125, 1, None, None)
    with pytest.raises(refused):
        lib.cs_step(C.byref(w32), 0.0125, 1.5, None, None)               # n_substeps
    with pytest.raises(refused):
        lib.cs_step(C.byref(w32), C.c_int(1), 1, None, None)             # dt
    with pytest.raises(refused):
        lib.cs_step(C.byref(w32), 0.0125, 1, None)                       # no stream
    assert lib.cs_step(C.byref(w32), 0.0125, 1, None, None) == _lib.CS_ERR_ARG      # the well-typed call gets as far as the library's own checks


def test_bare_addresses_reach_c_whole():
    """cs_value_net_pack (host only) with dims, the parameter-pointer array and the blob given as bare ints fills the bytes of the wrapped
    call -- with the blob above 4 GiB, where an address cut to 32 bits would not arrive."""
    import ctypes as C

    import numpy as np

    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(5)
    dims = np.array([1, 2, 9, 6, 2, 7, 5, 2, 4, 1, 2, 6, 1], np.int32)     # SARL with the global state: mlp1 9-6, mlp2 7-5, attention 4-1, mlp3 6-1
    ins = [13, 9, 6, 7, 12, 4, 11, 6]                                         # attention reads (mlp1, its mean) = 12, mlp3 (6 self columns, mlp2) = 11
    outs = [9, 6, 7, 5, 4, 1, 6, 1]
    arrays = [a for k, n in zip(ins, outs) for a in (rng.standard_normal((n, k)).astype(np.float32), rng.standard_normal(n).astype(np.float32))]
    ptrs = np.array([a.ctypes.data for a in arrays], np.uint64)
    nf = C.c_size_t(0)
    assert lib.cs_value_net_pack(1, dims.ctypes.data, len(dims), 13, None, None, C.byref(nf)) == 0, lib.cs_last_error()
    keep = []
    while True:                                                               # a few MiB: mmap-backed, high in the address space
        blob = np.full(max(nf.value, 1 << 20), np.float32(-7.0))
        if blob.ctypes.data >= 2 ** 32:
            break
        keep.append(blob)
        assert len(keep) < 64, "no allocation above 4 GiB"
    assert blob.ctypes.data >= 2 ** 32
    wrapped = np.full_like(blob, -7.0)
    assert lib.cs_value_net_pack(C.c_int(1), dims.ctypes.data_as(C.c_void_p), C.c_int(len(dims)), C.c_int(13), ptrs.ctypes.data_as(C.c_void_p),
                                 wrapped.ctypes.data_as(C.c_void_p), C.byref(nf)) == 0, lib.cs_last_error()
    assert lib.cs_value_net_pack(1, dims.ctypes.data, len(dims), 13, ptrs.ctypes.data, blob.ctypes.data, C.byref(nf)) == 0, lib.cs_last_error()
    assert np.any(wrapped[:nf.value] != -7.0)
    assert blob.tobytes() == wrapped.tobytes()


def test_library_on_disk_was_built_from_the_sources_on_disk():
    """The rebuild is keyed on a content hash of csrc/* + include/*: the id the LOADED library reports (cs_build_id) must
    be the hash of the sources in the tree, so a stale prebuilt .so cannot pass for the current code."""
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.csrc import build as hb

    st = hb.status()
    assert st["exists"] and st["fresh"], st
    lib = _lib.load()
    lib.cs_build_id.restype = C.c_char_p
    assert lib.cs_build_id().decode() == st["build_id"]
    # and the key really follows the content: a changed source gives a different id
    keys = hb.source_keys()
    assert hb.source_keys(["-DX"])["build_id"] != keys["build_id"]


def test_struct_layout_matches_header():
    import ctypes as C

    from social_navigation_pyenvs_amd._lib import cs_worlds

    # 8 int32 + 7 pointers + 5 floats + 2 int32 (+4 padding) + 1 pointer + 1 int32 (+4 padding) + 1 pointer + 1 int32 (+4 padding)
    assert C.sizeof(cs_worlds) == 8 * 4 + 7 * 8 + 5 * 4 + 2 * 4 + 4 + 8 + 4 + 4 + 8 + 4 + 4
    assert cs_worlds.d_state.offset == 32
    assert cs_worlds.orca_math.offset == C.sizeof(cs_worlds) - 8        # ABI 4: the ORCA arithmetic is a field of the context


def test_product_fails_loudly_without_gpu():
    from social_navigation_pyenvs_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    import numpy as np

    from social_navigation_pyenvs_amd.batched import CrowdWorlds

    with pytest.raises(_lib.CrowdstepError):
        CrowdWorlds(np.zeros((1, 2, 13)), np.zeros((1, 2, 1, 2)), np.zeros((2, 20)), type=0)


def test_header_is_plain_c_and_generator_struct_matches():
    """include/crowdstep.h is the contract a non-C++ host binds: it must compile as C, and the ctypes mirrors of its
    structs must have the compiler's layout."""
    import ctypes as C
    import subprocess
    import tempfile

    from social_navigation_pyenvs_amd._lib import cs_gym_book, cs_stage_book, cs_worlds
    from social_navigation_pyenvs_amd.generators import cs_generator

    src = ('#include "crowdstep.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cs_worlds), sizeof(cs_generator), '
           'offsetof(cs_generator, circle_radius), offsetof(cs_generator, robot_desired_speed), offsetof(cs_worlds, d_world_flags), offsetof(cs_worlds, d_orca_agent_params), '
           'sizeof(cs_gym_book), offsetof(cs_gym_book, clock_len), offsetof(cs_gym_book, d_reward), offsetof(cs_gym_book, seed_stride), '
           'sizeof(cs_stage_book), offsetof(cs_stage_book, d_failed), offsetof(cs_stage_book, depth));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes[0] == C.sizeof(cs_worlds)
    assert sizes[1] == C.sizeof(cs_generator)
    assert sizes[2] == cs_generator.circle_radius.offset
    assert sizes[3] == cs_generator.robot_desired_speed.offset
    assert sizes[4] == cs_worlds.d_world_flags.offset
    assert sizes[5] == cs_worlds.d_orca_agent_params.offset
    assert sizes[6] == C.sizeof(cs_gym_book) and sizes[7] == cs_gym_book.clock_len.offset and sizes[8] == cs_gym_book.d_reward.offset
    assert sizes[9] == cs_gym_book.seed_stride.offset
    assert sizes[10] == C.sizeof(cs_stage_book) and sizes[11] == cs_stage_book.d_failed.offset and sizes[12] == cs_stage_book.depth.offset


def test_integration_doc_stub_matches_the_struct():
    """The ctypes stub INTEGRATION.md shows a maintainer is the header's cs_worlds, field for field."""
    import ctypes as C

    from social_navigation_pyenvs_amd._lib import cs_worlds

    src = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"class cs_worlds\(C\.Structure\):.*?\n(    _fields_ = \[.*?\])\n", src, re.S)
    assert m, "stub not found"
    ns = {"C": C}
    exec("class stub(C.Structure):\n" + m.group(1), ns)
    stub = ns["stub"]
    assert [(f[0], f[1]) for f in stub._fields_] == [(f[0], f[1]) for f in cs_worlds._fields_]
    assert C.sizeof(stub) == C.sizeof(cs_worlds)


def test_hip_runtime_preload_checks_the_soname_and_maps_one_runtime(tmp_path, monkeypatch):
    """_lib.load() preloads torch's bundled libamdhip64 only when its SONAME is the one libcrowdstep.so NEEDs (so that the loader
    binds the library to it and a later `import torch` finds the same file mapped): exactly ONE libamdhip64 in /proc/self/maps here;
    a bundled runtime with another SONAME is not preloaded (a warning, the system runtime instead of two mapped runtimes)."""
    import subprocess
    import sys

    from social_navigation_pyenvs_amd import _lib

    _lib.load()
    soname, needed = _lib._elf_dynamic(_lib.LIB_PATH)
    want = [x for x in needed if x.startswith("libamdhip64")]
    assert len(want) == 1
    if _lib.hip_runtime_path:
        assert _lib._elf_dynamic(_lib.hip_runtime_path)[0] == want[0]
    assert len(_lib.mapped_hip_runtimes()) == 1, _lib.mapped_hip_runtimes()
    # a bundled runtime whose SONAME differs: simulated by pointing the check at a library that is not a HIP runtime at all
    code = ("import warnings, sys; sys.path.insert(0, %r)\n"
            "from social_navigation_pyenvs_amd import _lib\n"
            "real = _lib._elf_dynamic\n"
            "_lib._elf_dynamic = lambda p: ('libamdhip64.so.6', []) if 'torch' in p else real(p)\n"
            "with warnings.catch_warnings(record=True) as w:\n"
            "    warnings.simplefilter('always'); _lib.load()\n"
            "assert _lib.hip_runtime_path is None and any('not preloading' in str(x.message) for x in w), (_lib.hip_runtime_path, [str(x.message) for x in w])\n"
            "assert len(_lib.mapped_hip_runtimes()) == 1\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    subprocess.check_call([sys.executable, "-c", code])


def test_new_entry_points_reject_bad_arguments_before_touching_a_device():
    """Argument checks of the round-4 entry points come first: null pointers, a staging depth that is not a power of two, a staging
    batch of the wrong size, a generator that does not fit the worlds -- all CS_ERR_ARG (ValueError through the binding) with no GPU."""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.generators import cs_generator

    lib = _lib.load()
    null = C.c_void_p(None)
    assert lib.cs_gym_step(None, C.c_float(0.0125), C.c_int(20), null, C.c_float(0.25), null, null, null, None, C.c_int(0), null, null) == _lib.CS_ERR_ARG
    assert lib.cs_refill_staged_worlds(None, None, None, null) == _lib.CS_ERR_ARG
    assert lib.cs_consume_staged_worlds(None, None, None, null, None, C.c_int(0), null, null) == _lib.CS_ERR_ARG
    buf = C.create_string_buffer(8)
    assert lib.cs_device_pci_bus_id(C.c_int(0), buf, C.c_size_t(8)) == _lib.CS_ERR_ARG          # buffer too small for "0000:00:00.0"
    done = C.c_int(0)
    assert lib.cs_event_query(null, C.byref(done)) == _lib.CS_ERR_ARG
    # a well-formed descriptor pair with a bad stage book
    w = _lib.cs_worlds(W=8, n=5, G=2, type=3, layout=_lib.CS_LAYOUT_AOS, d_state=1, d_goals=1)
    st = _lib.cs_worlds(W=24, n=5, G=2, type=3, layout=_lib.CS_LAYOUT_AOS, d_state=1, d_goals=1)
    g = cs_generator(scenario=0, n=5, insert_robot=1, randomize_attributes=0, randomize_positions=1, max_tries=100, circle_radius=7.0,
                     traffic_length=14.0, traffic_height=3.0, robot_radius=0.3, human_mass=75.0, robot_mass=80.0, robot_desired_speed=1.0)
    book = _lib.cs_stage_book(d_seeds=1, d_base_seed=1, d_epoch=1, d_staged_seed=1, d_staged_status=1, d_failed=1, seed_stride=0, depth=3)
    assert lib.cs_refill_staged_worlds(C.byref(g), C.byref(st), C.byref(book), null) == _lib.CS_ERR_ARG   # depth 3: not a power of two
    assert "power of two" in lib.cs_last_error().decode()
    book.depth = 4
    mask = C.c_void_p(1)
    assert lib.cs_consume_staged_worlds(C.byref(g), C.byref(st), C.byref(w), mask, C.byref(book), C.c_int(0), null, null) == _lib.CS_ERR_ARG
    assert "differ in shape" in lib.cs_last_error().decode()                                             # 24 / 4 = 6 worlds staged per level, 8 live
    g.n = 7
    st.W = 32
    assert lib.cs_refill_staged_worlds(C.byref(g), C.byref(st), C.byref(book), null) == _lib.CS_ERR_ARG
    assert "cs_generator.n differs" in lib.cs_last_error().decode()


# One bad input per row, for every entry point that takes a cs_worlds: (entry, descriptor fields on top of a 4 x 5 SFM batch whose device
# pointers are all NULL, the status the library returns, a fragment of its message).  "dev" in the fields sets the four buffers d_state,
# d_goals, d_params, d_safety (and "robot" d_robot) to a dummy non-NULL address that the checks only compare with NULL; "book" = "null"
# hands over a cs_gym_book without buffers.  A row whose descriptor carries a dummy pointer into an entry that launches kernels is only run
# where no GPU is visible: nothing may ever hand such a pointer to a launch on a real device.
_ORCA = dict(type=9, orca_neighbor_dist=10.0, orca_time_horizon=5.0, orca_time_horizon_obst=5.0, orca_max_neighbors=10)
# worlds the Gym step takes in ONE launch on a 64-lane build (25 humans, Guo's SFM, CS_ALL_PARAMS_EQUAL, no walls), with one fault per row:
# "call" replaces one argument of the call (None, or a dummy address), "sb" / "book" = dict(...) one field of the cs_stage_book / cs_gym_book,
# "walls" adds one polygon (with a dummy d_obstacles)
_FUSED = dict(dev=1, robot=1, n=25, type=1, flags=1)
_STAGED_FAULTS = [
    (dict(_FUSED, sb=dict(d_pending=0)), "cs_gym_step_staged needs cs_stage_book.d_pending and d_failed"),
    (dict(_FUSED, sb=dict(d_failed=0)), "cs_gym_step_staged needs cs_stage_book.d_pending and d_failed"),
    (dict(_FUSED, book=dict(auto_reset=0)), "cs_gym_step_staged is the auto-reset step (cs_gym_book.auto_reset or the NEXT_STEP masks)"),
    (dict(_FUSED, book=dict(d_seeds=0x2000)), "cs_gym_book.d_seeds and cs_stage_book.d_seeds must be one buffer"),
    (dict(_FUSED, call=dict(gen=None)), "null argument"),
    (dict(_FUSED, call=dict(staging=None)), "null argument"),
    (dict(_FUSED, call=dict(sb=None)), "null argument"),
    (dict(_FUSED, walls=1), "cs_gym_step_staged: these worlds take the two launches (cs_gym_step, then cs_consume_staged_worlds)"),
]
_BAD_CS_WORLDS = [
    ("cs_step", None, -1, "null cs_worlds"),
    ("cs_step", dict(W=0), -1, "W, n, G must be positive"),
    ("cs_step", dict(n=0), -1, "W, n, G must be positive"),
    ("cs_step", dict(), -1, "null device buffer"),
    ("cs_step", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_step", dict(type=42), -2, "does not exist"),
    ("cs_step", dict(dev=1, O=1, Smax=2), -1, "bad obstacle description"),
    ("cs_step", dict(_ORCA), -1, "null device buffer"),
    ("cs_step", dict(_ORCA, W=0), -1, "W, n, G must be positive"),
    ("cs_step", dict(_ORCA, dev=1, orca_max_neighbors=17), -1, "orca_max_neighbors must be in 0..16"),
    ("cs_step", dict(type=10), -1, "null device buffer"),
    ("cs_step", dict(type=10, n=0), -1, "W, n, G must be positive"),
    ("cs_peek", None, -1, "null argument"),
    ("cs_peek", dict(W=0), -1, "W, n, G must be positive"),
    ("cs_peek", dict(), -1, "null device buffer"),
    ("cs_peek", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_peek", dict(type=42), -2, "does not exist"),
    ("cs_peek", dict(_ORCA, dev=1, orca_max_neighbors=17), -1, "orca_max_neighbors must be in 0..16"),
    ("cs_update_humans_parallel", None, -1, "null argument"),
    ("cs_update_humans_parallel", dict(n=0), -1, "W, n, G must be positive"),
    ("cs_update_humans_parallel", dict(), -1, "null device buffer"),
    ("cs_update_humans_parallel", dict(type=42), -2, "does not exist"),
    ("cs_update_humans_parallel", dict(dev=1, O=1, Smax=2), -1, "bad obstacle description"),
    ("cs_step_trace", None, -1, "null argument"),
    ("cs_step_trace", dict(W=0), -1, "W, n, G must be positive"),
    ("cs_step_trace", dict(), -1, "null device buffer"),
    ("cs_step_trace", dict(type=42), -1, "covers the SFM / HSFM models"),
    ("cs_step_trace", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_step_observe", None, -1, "null argument"),
    ("cs_step_observe", dict(n=0), -1, "W, n, G must be positive"),
    ("cs_step_observe", dict(), -1, "null device buffer"),
    ("cs_step_observe", dict(type=42), -2, "does not exist"),
    ("cs_step_observe", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_step_observe", dict(_ORCA, dev=1, orca_max_neighbors=17), -1, "orca_max_neighbors must be in 0..16"),
    ("cs_collision_reward", None, -1, "null cs_worlds"),
    ("cs_collision_reward", dict(W=0), -1, "bad cs_worlds"),
    ("cs_collision_reward", dict(n=0), -1, "bad cs_worlds"),
    ("cs_collision_reward", dict(), -1, "bad cs_worlds"),
    ("cs_collision_reward", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_collision_reward", dict(dev=1), -1, "null argument"),
    ("cs_collision_reward_gym", None, -1, "null argument"),
    ("cs_collision_reward_gym", dict(W=0), -1, "bad cs_worlds"),
    ("cs_collision_reward_gym", dict(), -1, "bad cs_worlds"),
    ("cs_collision_reward_gym", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_collision_reward_gym", dict(dev=1, robot=1, book="null"), -1, "null buffer in cs_gym_book"),
    ("cs_gym_step", None, -1, "null argument"),
    ("cs_gym_step", dict(W=0), -1, "bad cs_worlds"),
    ("cs_gym_step", dict(dev=1, robot=1, book="null"), -1, "null buffer in cs_gym_book"),
    ("cs_gym_step", dict(dev=1, robot=1, n=80, book="null"), -1, "null buffer in cs_gym_book"),
    ("cs_gym_step_staged", None, -1, "null argument"),
    ("cs_gym_step_staged", dict(W=0), -1, "these worlds take the two launches"),
    ("cs_gym_step_staged", dict(dev=1, robot=1, book="null"), -1, "null buffer in cs_gym_book"),
    ("cs_actual_collision_reward", None, -1, "null cs_worlds"),
    ("cs_actual_collision_reward", dict(n=0), -1, "bad cs_worlds"),
    ("cs_actual_collision_reward", dict(), -1, "bad cs_worlds"),
    ("cs_actual_collision_reward", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_robot_model_step", None, -1, "null cs_worlds"),
    ("cs_robot_model_step", dict(W=0), -1, "bad cs_worlds (a robot needs d_robot)"),
    ("cs_robot_model_step", dict(dev=1), -1, "bad cs_worlds (a robot needs d_robot)"),
    ("cs_robot_model_step", dict(dev=1, robot=1, layout=5), -1, "bad layout"),
    ("cs_robot_model_step", dict(dev=1, robot=1, O=1, Smax=2), -1, "bad obstacle description"),
    ("cs_robot_model_velocities", None, -1, "null cs_worlds"),
    ("cs_robot_model_velocities", dict(n=0), -1, "bad cs_worlds (a robot needs d_robot)"),
    ("cs_imitation_block", None, -1, "null cs_worlds"),
    ("cs_imitation_block", dict(W=0), -1, "bad cs_worlds (a robot needs d_robot)"),
    ("cs_robot_model_rk45", None, -1, "null cs_worlds"),
    ("cs_robot_model_rk45", dict(W=0), -1, "bad cs_worlds (a robot needs d_robot)"),
    ("cs_robot_model_rk45", dict(dev=1, robot=1, layout=5), -1, "bad layout"),
    ("cs_robot_model_rk45", dict(dev=1, robot=1, O=1, Smax=2), -1, "bad obstacle description"),
    ("cs_update_humans_rk45", None, -1, "null cs_worlds"),
    ("cs_update_humans_rk45", dict(type=42), -2, "does not exist"),
    ("cs_update_humans_rk45", dict(W=0), -1, "W, n, G must be positive"),
    ("cs_update_humans_rk45", dict(), -1, "null device buffer"),
    ("cs_update_humans_rk45", dict(dev=1, O=1, Smax=2), -1, "bad obstacle description"),
    ("cs_update_humans_rk45", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_complete_rk45_simulation", None, -1, "null cs_worlds"),
    ("cs_complete_rk45_simulation", dict(n=0), -1, "W, n, G must be positive"),
    ("cs_gym_observe", None, -1, "null argument"),
    ("cs_gym_observe", dict(), -1, "null argument"),
    ("cs_gym_observe", dict(dev=1, W=0), -1, "bad cs_worlds"),
    ("cs_gym_observe", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_copy_worlds_masked", None, -1, "null argument"),
    ("cs_copy_worlds_masked", dict(), -1, "null device buffer"),
    ("cs_copy_worlds_masked_status", None, -1, "null argument"),
    ("cs_copy_worlds_masked_observe", None, -1, "null argument"),
    ("cs_laser_scan", None, -1, "null argument"),
    ("cs_laser_scan", dict(W=0), -1, "bad cs_worlds"),
    ("cs_laser_scan", dict(), -1, "bad cs_worlds"),
    ("cs_laser_scan", dict(dev=1, O=1, Smax=2), -1, "bad obstacle description"),
    ("cs_laser_scan", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_laser_scan", dict(dev=1, n=0), -1, "no sensor pose"),          # n = 0 passes the laser's checks (the scan sees walls only)
    ("cs_generate_worlds", None, -1, "null argument"),
    ("cs_generate_worlds", dict(), -1, "null device buffer"),
    ("cs_generate_worlds", dict(dev=1, W=0), -1, "W, n, G must be positive"),
    ("cs_generate_worlds", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_refill_staged_worlds", None, -1, "null argument"),
    ("cs_refill_staged_worlds", dict(), -1, "null device buffer"),
    ("cs_consume_staged_worlds", None, -1, "null argument"),
    ("cs_consume_staged_worlds", dict(), -1, "null device buffer"),
    ("cs_reserve_scratch", None, -1, "null cs_worlds"),
    ("cs_launch_geometry", None, -1, "null cs_worlds"),
    ("cs_launch_geometry", dict(n=0), -1, "rows per world must be positive"),
    ("cs_step_variant", None, -1, "null argument"),
    ("cs_step_variant", dict(W=0), -1, "W, n, G must be positive"),
    ("cs_step_variant", dict(n=0), -1, "W, n, G must be positive"),
    ("cs_step_variant", dict(), -1, "null device buffer"),
    ("cs_step_variant", dict(dev=1, layout=5), -1, "bad layout"),
    ("cs_step_variant", dict(type=42), -2, "does not exist"),
    ("cs_step_variant", dict(dev=1, O=1, Smax=2), -1, "bad obstacle description"),
    # the register-resident ORCA build (maxNeighbors 10, no vertices) is the one whose name reports its arithmetic; cs_step_variant runs
    # orca_launch's checks, so an orca_math outside CS_ORCA_MATH_* is refused as the launch refuses it
    ("cs_step_variant", dict(_ORCA, dev=1, orca_math=3), 0, "math=fma"),
    ("cs_step_variant", dict(_ORCA, dev=1, orca_math=7), -1, "cs_worlds.orca_math"),
    ("cs_step_variant", dict(_ORCA, dev=1, orca_max_neighbors=17), -1, "orca_max_neighbors must be in 0..16"),
    # one fault per call on worlds that take the one-launch path (appended: the ids of the rows above carry their index)
    *[("cs_gym_step_staged", f, -1, m) for f, m in _STAGED_FAULTS],
    *[("cs_gym_step_staged_policy", f, -1, m) for f, m in _STAGED_FAULTS],
    ("cs_gym_step", dict(_FUSED, call=dict(action=None)), -1, "null argument"),
    ("cs_gym_step", dict(_FUSED, call=dict(out=None)), -1, "null argument"),
    ("cs_gym_step", dict(_FUSED, call=dict(cfg=None)), -1, "null argument"),
    ("cs_step_observe", dict(dev=1, n=25, type=1, flags=1, call=dict(action=0x1000)), -1, "robot action given but cs_worlds.d_robot is null"),
    ("cs_step_trace", dict(dev=1, n=25, type=1, flags=1, call=dict(action=0x1000)), -1, "robot action given but cs_worlds.d_robot is null"),
    # cs_lookahead takes no cs_worlds (the descriptor of the row is not handed over): its two argument checks behind the null pointers, both
    # before the launch -- 1920 actions fill the 60 KiB of LDS its frame table may take
    ("cs_lookahead", dict(call=dict(A=1921)), -1, "action set too large"),
    ("cs_lookahead", dict(call=dict(robot_stride=7)), -1, "robot rows need at least 8 columns"),
]
_QUERY_ENTRIES = {"cs_step_variant", "cs_launch_geometry", "cs_gym_step_is_one_launch"}


def _bad_cs_worlds_call(entry, w, book, sb_fields=None, over=None):
    """Calls `entry` with descriptor `w` (a ctypes pointer or None) and otherwise well-formed arguments: dummy device pointers for every
    buffer an entry checks for NULL before it reads the descriptor, host arrays for host arguments.  `sb_fields` changes fields of the
    cs_stage_book, `over` replaces named arguments of the Gym-step / step calls (None, or a dummy address)."""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.generators import cs_generator

    lib = _lib.load()
    null, dev = C.c_void_p(None), C.c_void_p(0x1000)
    f, i = C.c_float, C.c_int
    cfg = (C.c_float * 5)(25.0, 1.0, -0.25, 0.2, 0.5)
    rp = (C.c_float * 20)()
    gen = cs_generator(scenario=0, n=5, insert_robot=0, randomize_attributes=0, randomize_positions=1, max_tries=100, circle_radius=7.0,
                       traffic_length=14.0, traffic_height=3.0, robot_radius=0.3, human_mass=75.0, robot_mass=80.0, robot_desired_speed=1.0)
    sb = _lib.cs_stage_book(d_seeds=0x1000, d_base_seed=0x1000, d_epoch=0x1000, d_staged_seed=0x1000, d_staged_status=0x1000, d_failed=0x1000,
                            seed_stride=0, depth=1, d_pending=0x1000)
    for k, v in (sb_fields or {}).items():
        setattr(sb, k, v)
    over = over or {}
    ptr = lambda name, default: default if name not in over else (None if over[name] is None else C.c_void_p(over[name]))
    ref = lambda name, obj: None if name in over else (obj if name == "staging" else C.byref(obj))
    gb = C.byref(book)
    buf = C.create_string_buffer(256)
    gym = lambda: (w, f(0.01), i(1), ptr("action", dev), f(0.25), dev, ptr("cfg", cfg), ptr("out", dev), gb, i(0), dev)
    staged = lambda: (ref("gen", gen), ref("staging", w), ref("sb", sb))
    calls = {
        "cs_step": lambda: lib.cs_step(w, f(0.01), i(1), null, null),
        "cs_peek": lambda: lib.cs_peek(w, f(0.01), dev, null),
        "cs_update_humans_parallel": lambda: lib.cs_update_humans_parallel(w, f(0.01), dev, null),
        "cs_step_trace": lambda: lib.cs_step_trace(w, f(0.01), i(1), ptr("action", null), dev, null),
        "cs_step_observe": lambda: lib.cs_step_observe(w, f(0.01), i(1), ptr("action", null), i(0), dev, null),
        "cs_collision_reward": lambda: lib.cs_collision_reward(w, dev, f(0.25), dev, cfg, dev, null),
        "cs_collision_reward_gym": lambda: lib.cs_collision_reward_gym(w, dev, f(0.25), dev, cfg, dev, gb, null),
        "cs_gym_step": lambda: lib.cs_gym_step(*gym(), null),
        "cs_gym_step_staged": lambda: lib.cs_gym_step_staged(*gym(), *staged(), null),
        "cs_gym_step_staged_policy": lambda: lib.cs_gym_step_staged_policy(*gym(), *staged(), i(0), f(0.25), None, null),   # CS_PNT_BP: no parameters
        "cs_actual_collision_reward": lambda: lib.cs_actual_collision_reward(w, f(0.25), dev, cfg, dev, null),
        "cs_robot_model_step": lambda: lib.cs_robot_model_step(w, i(0), rp, f(0.0), dev, dev, f(0.01), null),
        "cs_robot_model_velocities": lambda: lib.cs_robot_model_velocities(w, i(0), rp, f(0.0), dev, dev, f(0.01), null),
        "cs_imitation_block": lambda: lib.cs_imitation_block(w, i(0), rp, f(0.0), dev, dev, f(0.01), i(1), null),
        "cs_robot_model_rk45": lambda: lib.cs_robot_model_rk45(w, i(0), rp, f(0.0), dev, dev, f(0.01), null, null),
        "cs_update_humans_rk45": lambda: lib.cs_update_humans_rk45(w, f(0.01), dev, null, null),
        "cs_complete_rk45_simulation": lambda: lib.cs_complete_rk45_simulation(w, f(0.01), f(1.0), dev, dev, i(4), null, null),
        "cs_gym_observe": lambda: lib.cs_gym_observe(w, i(0), dev, null),
        "cs_copy_worlds_masked": lambda: lib.cs_copy_worlds_masked(w, w, dev, null),
        "cs_copy_worlds_masked_status": lambda: lib.cs_copy_worlds_masked_status(w, w, dev, null, null),
        "cs_copy_worlds_masked_observe": lambda: lib.cs_copy_worlds_masked_observe(w, w, dev, null, i(0), null, null),
        "cs_laser_scan": lambda: lib.cs_laser_scan(w, null, i(0), f(6.28), i(16), f(10.0), dev, null),
        "cs_generate_worlds": lambda: lib.cs_generate_worlds(C.byref(gen), w, dev, null, null, null, dev, null),
        "cs_refill_staged_worlds": lambda: lib.cs_refill_staged_worlds(C.byref(gen), w, C.byref(sb), null),
        "cs_consume_staged_worlds": lambda: lib.cs_consume_staged_worlds(C.byref(gen), w, w, dev, C.byref(sb), i(0), null, null),
        "cs_reserve_scratch": lambda: lib.cs_reserve_scratch(w, i(1), null),
        "cs_launch_geometry": lambda: lib.cs_launch_geometry(w, null, null, null),
        "cs_step_variant": lambda: lib.cs_step_variant(w, i(0), buf, C.c_size_t(len(buf))),
        "cs_lookahead": lambda: lib.cs_lookahead(i(3), i(5), i(over.get("A", 81)), i(0), dev, dev, dev, dev, i(over.get("robot_stride", 9)), f(0.25), dev, dev, null),
    }
    rc = calls[entry]()
    return rc, (buf.value if entry == "cs_step_variant" and rc == 0 else lib.cs_last_error()).decode()


@pytest.mark.parametrize("entry,fields,rc,fragment", _BAD_CS_WORLDS,
                         ids=[f"{r[0]}-{i}" for i, r in enumerate(_BAD_CS_WORLDS)])
def test_cs_worlds_entry_points_check_their_arguments(entry, fields, rc, fragment):
    """What every entry point that takes a cs_worlds answers to one bad input -- the status and the message -- with no GPU involved."""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib

    sb_fields = over = None
    w, book = None, _lib.cs_gym_book(**{k: 0x1000 for k in ("d_counter", "d_seeds", "d_mask", "d_clock", "d_reward", "d_terminated",
                                                            "d_truncated", "d_info")}, clock_len=4, auto_reset=1)
    if fields is not None:
        fields = dict(fields)
        dummy = fields.pop("dev", 0)
        robot = fields.pop("robot", 0)
        book_fields = fields.pop("book", None)
        if book_fields == "null":
            book = _lib.cs_gym_book(clock_len=4, auto_reset=1)
        else:
            for k, v in (book_fields or {}).items():
                setattr(book, k, v)
        sb_fields, over, walls = fields.pop("sb", None), fields.pop("call", None), fields.pop("walls", 0)
        desc = _lib.cs_worlds(**{"W": 4, "n": 5, "G": 2, "type": 0, "layout": _lib.CS_LAYOUT_AOS, **fields})
        if dummy:
            desc.d_state = desc.d_goals = desc.d_params = desc.d_safety = 0x1000
        if walls:
            desc.O, desc.Smax, desc.d_obstacles = 1, 4, 0x1000
        if robot:
            desc.d_robot = 0x1000
        if (dummy or robot) and entry not in _QUERY_ENTRIES and _lib.device_count() > 0:
            pytest.skip("a GPU is visible: a dummy device pointer is never handed to an entry point that launches kernels there")
        w = C.byref(desc)
    got_rc, msg = _bad_cs_worlds_call(entry, w, book, sb_fields, over)
    assert (got_rc, fragment in msg) == (rc, True), msg
