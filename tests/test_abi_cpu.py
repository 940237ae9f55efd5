"""CPU-side checks of the product boundary: libkmc.so loads and exports every symbol that
include/kmc.h declares, the ctypes structs match the header, kernels specialise for gfx950
without a GPU, bad constants are rejected, the library fails loudly without a device, and the
host-side pack/unpack/fingerprint logic round-trips (no compute calls: there is no GPU here)."""
import ctypes as C
import json
import os
import random
import re

import pytest

import kmo
from kafka_specification_amd import CheckerConfig, KmcError, ModelChecker, precompile
from kafka_specification_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "kmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(kmc_[a-z_0-9]+)\s*\(", text)) - {"kmc_progress_cb"})


TUNING_LIB = os.path.join(os.path.dirname(nat.LIB_PATH), "libkmc_tuning.so")   # the same engine + the tuning aids (csrc/Makefile)
CSRC = os.path.join(ROOT, "kafka_specification_amd", "csrc")


def test_library_exports_every_declared_symbol():
    names = header_functions()
    assert len(names) >= 25
    for path in (nat.LIB_PATH, TUNING_LIB):
        lib = C.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{os.path.basename(path)} does not export {n}"
    assert sorted(n for n, _, _ in nat.SYMBOLS) == names  # the binding covers exactly the header


def test_the_tuning_aids_are_in_the_tuning_library_only():
    """The dry / shadow passes (their report line) live in libkmc_tuning.so and not in libkmc.so, and the buffer-moving
    experiment that leaked device memory on purpose is in neither.  (Neither string occurs in the device source both embed.)"""
    shipped, tuning = open(nat.LIB_PATH, "rb").read(), open(TUNING_LIB, "rb").read()
    assert b"dry/shadow expand" not in shipped and b"dry/shadow expand" in tuning
    assert b"KMC_DEBUG_REALLOC" not in shipped and b"KMC_DEBUG_REALLOC" not in tuning


def _readme_table_names(heading):
    """The KMC_* names that open a first-column cell of the table under `heading` of README.md."""
    text = open(os.path.join(ROOT, "README.md")).read()
    assert text.count("\n### " + heading) == 1, heading
    section = text.split("\n### " + heading, 1)[1].split("\n#", 1)[0]
    rows = [l for l in section.splitlines() if l.startswith("| `")]
    return {m for l in rows for m in re.findall(r"`(KMC_[A-Z0-9_]+)", l.split(" | ")[0])}


def test_the_environment_the_engine_reads_is_the_environment_the_readme_names():
    """Every KMC_* variable handed to getenv / the env_* helpers (csrc/kmc_engine_internal.h) by the units of libkmc.so is a row
    of README's "Environment the library honours", and the other way round; the same for kmc_engine_tuning.cpp and the "Tuning
    build" table; and no unit keeps a value of the environment in a function-local static, where a handle opened later would
    not see it change."""
    import glob
    read = re.compile(r'\b(?:getenv|env_str|env_int|env_flag)\(\s*"(KMC_[A-Z0-9_]+)"')
    units = sorted(glob.glob(os.path.join(CSRC, "kmc_engine_*.cpp")))
    assert len(units) == 7
    shipped, tuning = set(), set()
    for path in units:
        text = open(path).read()
        (tuning if path.endswith("kmc_engine_tuning.cpp") else shipped).update(read.findall(text))
        assert not [l for l in text.splitlines() if "static const" in l and "getenv" in l], path
        assert "getenv" not in text, path           # (the helpers are the only callers: kmc_engine_internal.h)
    assert shipped == _readme_table_names("Environment the library honours") and len(shipped) == 12, sorted(shipped)
    assert tuning == _readme_table_names("Tuning build") and len(tuning) == 6, sorted(tuning)
    assert not shipped & tuning


def test_struct_sizes_match_header_layout():
    # kmc_config: 6*i32 + i64 + u32 + 6*i32 + (pad) + 5*u64 + ptr + 2*i32 ; kmc_result: see header
    assert C.sizeof(nat.KmcConfig) == 120
    assert C.sizeof(nat.KmcLevelInfo) == 40 + 8 * 16 + 32 + 32 + 32 + 32 + 8 + 8 + 8
    assert C.sizeof(nat.KmcResult) == 8 * 4 + 8 + 8 + 32 + 8 + 8 + 8 * 16 + 8 * 3 + 16 + 8 + 16 + 8 + 8 + 8 * 3
    assert C.sizeof(nat.KmcLevelStat) == 8 * 4 + 8 * 16 + 8 * 2 + 8 * 2
    # ... and the native front end, compiled against the header itself, agrees (it prints sizeof of both with -abi-sizes)
    import subprocess
    exe = os.path.join(ROOT, "kafka_specification_amd", "tlc")
    out = subprocess.run([exe, "-abi-sizes"], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(nat.KmcConfig), C.sizeof(nat.KmcLevelInfo), C.sizeof(nat.KmcResult),
                                     C.sizeof(nat.KmcLevelStat), C.sizeof(nat.KmcTiming)]


def test_names():
    lib = nat.lib()
    assert lib.kmc_model_name(5) == b"Kip320" and lib.kmc_invariant_name(2) == b"StrongIsr"
    assert [lib.kmc_action_name(5, k) for k in range(9)][7] == b"FencedBecomeFollowerAndTruncate"
    assert lib.kmc_action_name(2, 7) == b"BecomeFollowerTruncateToHighWatermark"
    assert lib.kmc_action_count(6) == 10 and lib.kmc_action_name(6, 9) == b"FollowerTruncate"
    assert lib.kmc_action_count(1) == 3 and lib.kmc_action_count(0) == 1
    assert lib.kmc_model_name(7) == b"AsyncIsr" and lib.kmc_action_count(7) == 7
    assert lib.kmc_action_name(7, 1) == b"ControllerHandleRequest" and lib.kmc_action_name(7, 6) == b"FollowerReplicate"
    assert lib.kmc_model_invariant_name(7, 1) == b"ValidHighWatermark" and lib.kmc_model_invariant_name(5, 1) == b"WeakIsr"


def test_specialises_for_gfx950_without_a_gpu(tmp_path):
    cfg = CheckerConfig(model="Kip101", n_replicas=2, log_size=3, max_records=2, max_leader_epoch=1,
                        cache_dir=str(tmp_path))
    precompile(cfg, "gfx950", 0)       # the search's own code object ...
    objects = lambda: [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]
    files = objects()
    assert len(files) == 1 and files[0].startswith("Kip101_N2_L3_R2_E1-gfx950-")
    assert open(os.path.join(tmp_path, files[0]), "rb").read(4) == b"\x7fELF"
    # ... and who compiled it, IN ITS NAME: two compilers can never write one file
    from kafka_specification_amd import compiler_identity
    mine = compiler_identity(0)
    assert mine > 0 and files[0].endswith(f"-c{mine}.hsaco")
    precompile(cfg, "gfx950")          # ... and all three: k_expand for the level-step interface and as an enumerator beside it
    files = sorted(objects(), key=len)
    assert len(files) == 3 and files[1].endswith("-enum.hsaco") and files[2].endswith("-sharded.hsaco")
    assert all(f.startswith("Kip101_N2_L3_R2_E1-gfx950-") for f in files)
    with pytest.raises(KmcError):
        precompile(cfg, "gfx950", 3)


@pytest.mark.parametrize("kw", [dict(model="Kip320", n_replicas=9), dict(model="Kip320", n_replicas=1),
                                dict(model="Kip320", log_size=20, max_records=30, max_leader_epoch=7),
                                dict(model="Kip320", max_leader_epoch=8), dict(model="IdSequence", max_id=-1)])
def test_bad_constants_are_rejected(kw):
    with pytest.raises(KmcError) as e:
        precompile(CheckerConfig(**kw))
    assert e.value.code == 1  # KMC_E_ARG


def test_open_fails_loudly_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(KmcError) as e:
        ModelChecker(CheckerConfig(model="Kip320"))
    assert e.value.code == 2 and "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("model,N,L,R,E", [("Kip320", 3, 6, 6, 2), ("Kip279", 5, 2, 2, 2), ("Kip320", 7, 8, 8, 3),
                                           ("Kip101", 2, 3, 3, 1)])
def test_pack_unpack_roundtrip_on_reachable_states(model, N, L, R, E):
    # reachable states from the oracle -> packed words -> canonical bytes; distinct states must
    # get distinct words (the packing is injective) and survive the round trip
    o = kmo.Run(kmo.make_config(model, N=N, L=L, R=R, E=E, invariants=(), max_states=3000, threads=2))
    n = min(o.distinct, 3000)
    with ModelChecker(CheckerConfig(model=model, n_replicas=N, log_size=L, max_records=R, max_leader_epoch=E,
                                    device=-1)) as mc:
        assert mc.canon_bytes == o.sb
        seen = {}
        rng = random.Random(1)
        for idx in rng.sample(range(n), min(n, 400)):
            b = o.state(idx)
            w = tuple(mc.pack(b))
            assert mc.unpack(w) == b
            assert seen.setdefault(w, b) == b
            assert mc.fingerprint(w) != 0
        init = mc.pack(o.state(0))
        assert sum(1 for x in init if x) == 1  # Init: everything zero except quorumState.isr = Replicas


def test_host_only_handle_cannot_run():
    with ModelChecker(CheckerConfig(model="Kip320", device=-1)) as mc:
        with pytest.raises(KmcError) as e:
            mc.run()
        assert e.value.code == 5


def test_fingerprint_avalanche_on_structured_states():
    # The fingerprint (shared host/device source, csrc/kmc_device.h) must fully avalanche: packed
    # states differ in a handful of low-entropy bits, and a weak per-word mix produced systematic
    # collisions at 75 M states.  Flip every input bit of reachable states: each output bit must
    # flip with probability ~1/2, and single-bit neighbours must never collide.
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=6, R=6, E=2, invariants=(), max_states=2000, threads=2))
    with ModelChecker(CheckerConfig(model="Kip320", n_replicas=3, log_size=6, max_records=6, max_leader_epoch=2,
                                    device=-1)) as mc:
        import numpy as np
        W = mc.state_words
        rows = []
        for idx in range(0, min(o.distinct, 2000), 5):
            w = mc.pack(o.state(idx))
            f0 = mc.fingerprint(w)
            row = []
            for k in range(W):
                for b in range(64):
                    w2 = list(w)
                    w2[k] ^= 1 << b
                    row.append(f0 ^ mc.fingerprint(w2))
            rows.append(row)
    d = np.array(rows, dtype=np.uint64)                      # [samples, 64*W]
    assert (d != 0).all()
    bits = ((d[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(np.float64)
    rate = bits.mean(axis=0)                                 # [input bit, output bit] flip probability
    samples = d.shape[0]
    sigma = 0.5 / samples ** 0.5
    assert np.abs(rate - 0.5).max() < 6 * sigma, (np.abs(rate - 0.5).max(), sigma)


def test_fingerprints_are_distinct_on_a_reachable_set():
    # 176,440 reachable states of Kip320 3/3/3/1: all fingerprints distinct, for two seeds
    o = kmo.Run(kmo.make_config("Kip320", N=3, L=3, R=3, E=1, invariants=(), threads=4))
    for seed in (0, 0xDEADBEEF):
        with ModelChecker(CheckerConfig(model="Kip320", n_replicas=3, log_size=3, max_records=3, max_leader_epoch=1,
                                        device=-1, hash_seed=seed)) as mc:
            fps = set()
            for idx in range(0, o.distinct, 3):
                fps.add(mc.fingerprint(mc.pack(o.state(idx))))
            assert len(fps) == len(range(0, o.distinct, 3))


def test_pack_unpack_property_random_fields():
    """hypothesis: for random constants and random in-range field values, unpack(pack(x)) == x and
    distinct canonical states get distinct packed words (the layout shared by host and device)."""
    from hypothesis import given, settings, strategies as st

    @st.composite
    def case(draw):
        N = draw(st.integers(2, 8)); E = draw(st.integers(0, 7)); R = draw(st.integers(1, 12))
        bits_rec = max(1, (E).bit_length() if E else 0) + (R + 1 - 1).bit_length()
        L = draw(st.integers(1, max(1, min(10, 64 // max(1, (R).bit_length() + (E).bit_length() or 1)))))
        return N, L, R, E, draw(st.randoms(use_true_random=False))

    handles = {}

    @settings(max_examples=120, deadline=None)
    @given(case())
    def run(c):
        N, L, R, E, rnd = c
        key = (N, L, R, E)
        if key not in handles:
            try:
                handles[key] = ModelChecker(CheckerConfig(model="Kip320", n_replicas=N, log_size=L, max_records=R,
                                                          max_leader_epoch=E, device=-1))
            except KmcError:
                handles[key] = None     # constants that cannot be packed are rejected, not mis-packed
        mc = handles[key]
        if mc is None:
            return
        b = bytearray()
        for _ in range(N):
            end = rnd.randint(0, L)
            b += bytes([end, rnd.randint(0, L), rnd.randint(0, E + 1), rnd.randint(0, N), rnd.randint(0, (1 << N) - 1)])
            b += bytes((1 + rnd.randint(0, R - 1) * (E + 1) + rnd.randint(0, E)) if o < end else 0 for o in range(L))
        nep = rnd.randint(0, E + 1)
        b += bytes([rnd.randint(0, R), nep, rnd.randint(0, E + 1), rnd.randint(0, N), rnd.randint(0, (1 << N) - 1)])
        for e in range(E + 1):
            b += bytes([rnd.randint(0, N), rnd.randint(0, (1 << N) - 1)]) if e < nep else bytes([0, 0])
        b = bytes(b)
        assert len(b) == mc.canon_bytes
        w = mc.pack(b)
        assert mc.unpack(w) == b
        assert len(w) == mc.state_words and all(0 <= x < 1 << 64 for x in w)
        b2 = bytearray(b); b2[1] = (b2[1] + 1) % (L + 1)      # change one field (hw of replica 0)
        if bytes(b2) != b:
            assert mc.pack(bytes(b2)) != w

    run()
    for mc in handles.values():
        if mc is not None:
            mc.close()


def test_async_isr_pack_unpack_property_random_fields():
    """hypothesis, AsyncIsr layout: random constants and random in-range field values — including the one
    spare value per bounded field that a successor outside the state constraint carries — round-trip
    through pack/unpack, and flipping one request bit changes the packed words."""
    from hypothesis import given, settings, strategies as st

    handles = {}

    @settings(max_examples=120, deadline=None)
    @given(st.integers(1, 6), st.integers(1, 40), st.integers(0, 7), st.randoms(use_true_random=False))
    def run(N, M, V, rnd):
        key = (N, M, V)
        if key not in handles:
            handles[key] = ModelChecker(CheckerConfig(model="AsyncIsr", n_replicas=N, log_size=M, max_leader_epoch=V,
                                                      device=-1))
        mc = handles[key]
        full = (1 << N) - 1
        rb = ((1 << N) + 7) // 8
        cver = rnd.randint(0, V + 1)
        b = bytearray([rnd.randint(0, full), cver, rnd.randint(0, full), rnd.randint(0, V), rnd.randint(0, full),
                       rnd.randint(0, V + 1)])
        b += bytes(rnd.randint(0, M + 1) for _ in range(N))
        req = bytearray((V + 1) * rb)
        for v in range(V + 1):
            for mask in range(1 << N):
                if rnd.random() < 0.2:
                    req[v * rb + (mask >> 3)] |= 1 << (mask & 7)
        b += req
        b += bytes(rnd.randint(1, full) if v < cver else 0 for v in range(V + 1))
        b = bytes(b)
        assert len(b) == mc.canon_bytes == 6 + N + (V + 1) * rb + V + 1
        w = mc.pack(b)
        assert mc.unpack(w) == b and len(w) == mc.state_words
        b2 = bytearray(b)
        b2[6 + N] ^= 1                                    # the request [isr {}, version 0]
        assert mc.pack(bytes(b2)) != w

    run()
    for mc in handles.values():
        mc.close()


def test_no_cached_expand_kernel_spills_vector_registers():
    """The register budget follows the kernel (kmc_engine_codeobj.cpp, get_code_object): k_expand is recompiled
    with fewer waves per SIMD until it spills at most 8 VGPRs.  At 184 spilled VGPRs the 7-replica Kip320
    kernel lost successors, so every code object the build step cached is checked here."""
    import glob
    import shutil
    import subprocess
    readelf = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    files = glob.glob(os.path.join(ROOT, "kafka_specification_amd", "kmc_cache", "*.hsaco"))
    if not files:
        pytest.skip("kernel cache not populated (python __graft_entry__.py)")
    seen_wide = False
    for f in files:
        notes = subprocess.run([readelf, "--notes", f], capture_output=True, text=True).stdout
        blocks = notes.split(".name:")[1:]
        # one k_expand per code object (round 5: a mode each — the search's, `-sharded`, `-enum`); a tuning / verify build
        # of the search's object also carries the dry kernel
        expand = [b for b in blocks if b.strip().startswith("kmc_expand_")]
        assert 1 <= len(expand) <= 2 and (len(expand) == 1 or any(b.strip().startswith("kmc_expand_dry_") for b in expand)), f
        tag = "_sh_" if f.endswith("-sharded.hsaco") else "_en_" if f.endswith("-enum.hsaco") else None
        assert all(b.strip().startswith("kmc_expand" + tag) for b in expand) if tag else \
            not any(b.strip().startswith(("kmc_expand_sh_", "kmc_expand_en_")) for b in expand), f
        for blk in expand:
            spills = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1))
            vgprs = int(re.search(r"\.vgpr_count:\s*(\d+)", blk).group(1))
            if not blk.strip().startswith("kmc_expand_dry_"):   # (the rule is applied to the kernel a search runs)
                assert spills <= 8, f"{os.path.basename(f)}: k_expand spills {spills} VGPRs at {vgprs}"
            seen_wide = seen_wide or vgprs > 128
    assert seen_wide   # the wide-replica kernels did get the larger budget


def test_the_search_kernel_takes_its_own_argument_block_and_holds_no_other_mode():
    """Round 5: k_expand is one kernel per mode.  The search's own kernel receives KmcArgsLocal — 168 bytes
    where the four-mode kernel of round 4 took 248 — and its scalar-register spills are what is left of one mode's code:
    the headline's object reported 286 spilled SGPRs / 770 v_readlane in round 4 (profiles/r05_mode_split.txt)."""
    import shutil
    import subprocess
    readelf = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not (os.path.exists(readelf) and os.path.exists(objdump)):
        pytest.skip("llvm-readelf / llvm-objdump not available")
    from kafka_specification_amd import code_object_path
    cfg = CheckerConfig(model="Kip320", n_replicas=3, log_size=6, max_records=6, max_leader_epoch=2)
    path = code_object_path(cfg)
    notes = subprocess.run([readelf, "--notes", path], capture_output=True, text=True).stdout
    blk = [b for b in notes.split(".name:")[1:] if b.strip().startswith("kmc_expand_Kip320")]
    assert len(blk) == 1
    # the metadata lists a kernel's keys alphabetically: .kernarg_segment_size precedes .name
    head = notes.split(".name:")[0:1 + [b.strip().startswith("kmc_expand_Kip320") for b in notes.split(".name:")[1:]].index(True)][-1]
    kernarg = int(re.findall(r"\.kernarg_segment_size:\s*(\d+)", head)[-1])
    assert kernarg == 168 + 256, kernarg            # KmcArgsLocal + the hidden arguments
    assert int(re.search(r"\.sgpr_spill_count:\s*(\d+)", blk[0]).group(1)) <= 160
    text = subprocess.run([objdump, "-d", path], capture_output=True, text=True, check=True).stdout
    body = text.split("<kmc_expand_Kip320_N3_L6_R6_E2>:")[1].split(">:")[0]
    assert body.count("v_readlane_b32") <= 200
    names = re.findall(r"<(kmc_\w+)>:", text)
    assert not any(n.startswith(("kmc_expand_sh_", "kmc_expand_en_", "kmc_expand_dry_")) for n in names)
    assert any(n.startswith("kmc_inv_") for n in names)


@pytest.mark.parametrize("defines", ["-DKMC_PROFILE=1", "-DKMC_FAULT_DROP=1", "-DKMC_TEST_FP_BITS=10", "-DKMC_FOLD_MIN_WORDS=4"])
def test_a_diagnostic_define_without_a_tuning_build_fails_loudly(tmp_path, monkeypatch, defines):
    """csrc/kmc_common.h: the diagnostic switches only exist in a -DKMC_TUNING=1 build (a stale script asking for one
    without it must not run a normal kernel under another cache key and pass vacuously), and the fingerprint's fold threshold is
    shared with the host, which computes fingerprints for `contains`, traces and checkpoints: a device build cannot be given
    another one behind its back.  Asked for plainly, each is a compile error, not a cached object."""
    monkeypatch.setenv("KMC_JIT_DEFINES", defines)
    cfg = CheckerConfig(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1, cache_dir=str(tmp_path))
    with pytest.raises(KmcError) as e:
        precompile(cfg, "gfx950", 0)
    assert "tuning build" in str(e.value)
    assert not any(f.endswith(".hsaco") for f in os.listdir(tmp_path))


def test_the_cache_key_names_the_compiler_and_every_process_prefers_the_pinned_one(tmp_path, monkeypatch):
    """The code-object cache (csrc/kmc_engine_codeobj.cpp): the compiler's identity is part of the file name, a process bound to
    ANOTHER compiler loads the pinned compiler's object when the cache holds it (the bench under PyTorch's runtime and a rocprofv3
    run under the system's execute the same machine code), compiles its own — under its own name — when it does not, and never
    touches the other's file."""
    import subprocess
    import sys
    code = ("import sys, os; sys.path.insert(0, %r); import kafka_specification_amd as kmc; "
            "c = kmc.CheckerConfig(model='Kip320', n_replicas=2, log_size=1, max_records=1, max_leader_epoch=1, cache_dir=%r); "
            "print(kmc.compiler_identity(0), kmc.compiler_identity(1), kmc.code_object_path(c))" % (ROOT, str(tmp_path)))

    def run(**env):   # a fresh process: which HIP runtime (and with it which hiprtc / comgr) it binds is decided at its first import
        e = {k: v for k, v in os.environ.items() if k not in ("KMC_NO_TORCH", "KMC_COMPILER_PIN", "KMC_JIT_DEFINES")}
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(e, **env), check=True).stdout.split()
        return int(out[0]), int(out[1]), out[2]

    torch_id, pinned, p1 = run()                         # PyTorch imported first: its bundled runtime
    assert pinned == 70051831 == torch_id                # csrc/kmc_engine_internal.h, KMC_PINNED_COMPILER (profiles/r06_compiler_ab.txt)
    assert re.search(rf"-c{torch_id}\.hsaco$", p1)
    blob = open(p1, "rb").read()
    sys_id, _, p2 = run(KMC_NO_TORCH="1")                # the system ROCm's runtime, same cache
    assert sys_id != torch_id, "this image should hold two HIP runtimes (PyTorch's bundle and /opt/rocm)"
    assert p2 == p1                                      # ... loads the pinned compiler's object
    sys_id2, pin2, p3 = run(KMC_NO_TORCH="1", KMC_COMPILER_PIN="0")   # no preference: it compiles its own, under its own name
    assert sys_id2 == sys_id and pin2 == 0
    assert p3 != p1 and p3.endswith(f"-c{sys_id}.hsaco") and os.path.exists(p3)
    assert open(p1, "rb").read() == blob                 # and never touches the other's file
    assert sorted(os.listdir(tmp_path)) == sorted({os.path.basename(p1), os.path.basename(p3)})
    _, _, p4 = run(KMC_COMPILER_PIN=str(sys_id))         # pinned to the system's: PyTorch's process now loads THAT object
    assert p4 == p3


def test_deferred_probe_load_is_issued_at_the_defer_point(tmp_path):
    """the deferred probe's first load (kmc_expand_body, `pd_v = a.table[i]`) must be ISSUED where the batch is
    deferred — ahead of the walk's leaves it is supposed to hide under — not sunk next to the compare-and-swap that consumes it.
    In the ISA of a build that defers (forced onto a small configuration): inside the flush, after the fingerprint's last
    multiply there is a global_load of the slot BEFORE the next LDS write of the successor ring / the next s_cbranch back into
    the walk, and the cmpswap that follows it is separated from it by other work."""
    import subprocess
    cfg = CheckerConfig(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1, cache_dir=str(tmp_path))
    os.environ["KMC_JIT_DEFINES"] = "-DKMC_DEFER_MIN_WORDS=1"
    try:
        from kafka_specification_amd import code_object_path
        path = code_object_path(cfg)
    finally:
        del os.environ["KMC_JIT_DEFINES"]
    asm = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True,
                         check=True).stdout
    body = asm[asm.index("<kmc_expand_Kip320_N3_L2_R2_E1>:"):]
    body = body[:body.index("\n\n", 10)] if "\n\n" in body[10:] else body
    lines = [ln.split("//")[0].strip() for ln in body.splitlines()]
    ops = [ln.split()[0] for ln in lines if ln and not ln.endswith(":") and not ln.startswith("<")]
    cas = [i for i, o in enumerate(ops) if o.startswith("global_atomic_cmpswap")]
    assert cas, "no compare-and-swap in the search's kernel?"
    # every claim is preceded by a probe load; for the DEFERRED claim the nearest preceding 8-byte global load of a table slot
    # lies far upstream (the whole walk is between them): at least one cmpswap whose previous global_load_dwordx2 is more than
    # 200 instructions back, with LDS ring writes (ds_write) in between
    def gap(i):
        for j in range(i - 1, -1, -1):
            if ops[j].startswith("global_load_dwordx2"):
                return i - j, sum(1 for o in ops[j:i] if o.startswith("ds_write"))
        return 0, 0
    gaps = [gap(i) for i in cas]
    assert any(g > 200 and w > 0 for g, w in gaps), gaps


def test_a_probe_step_sends_the_claims_and_the_next_loads_together(tmp_path):
    """KmcSink::claim_steps (round 6): in one step of a wave's walk the lanes that saw an empty slot send their compare-and-swap
    and the lanes that must walk on send the load of their next slot, and the wave waits ONCE for both.  Nothing in the language
    says so — a `s_waitcnt vmcnt(0)` between the two requests would turn the step back into the textbook loop's two round
    trips — so the ISA is read: in the search's kernel every probe-loop compare-and-swap is followed by a global load of a table
    slot before the next wait on the vector-memory counter."""
    import subprocess
    cfg = CheckerConfig(model="Kip320", n_replicas=3, log_size=2, max_records=2, max_leader_epoch=1, cache_dir=str(tmp_path))
    from kafka_specification_amd import code_object_path
    path = code_object_path(cfg)
    asm = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True,
                         check=True).stdout
    body = asm[asm.index("<kmc_expand_Kip320_N3_L2_R2_E1>:"):]
    body = body[:body.index("\n\n", 10)] if "\n\n" in body[10:] else body
    lines = [ln.split("//")[0].strip() for ln in body.splitlines()]
    ins = [ln for ln in lines if ln and not ln.endswith(":") and not ln.startswith("<")]
    cas = [i for i, o in enumerate(ins) if o.startswith("global_atomic_cmpswap")]
    assert len(cas) >= 3, "the narrow, the paired (fingerprint + predecessor) and the wide walk each hold one compare-and-swap"
    for i in cas:
        nxt = next(j for j in range(i + 1, len(ins)) if ins[j].startswith("s_waitcnt") and "vmcnt" in ins[j])
        between = [o.split()[0] for o in ins[i + 1:nxt]]
        assert any(o.startswith("global_load_dwordx") for o in between), (ins[i], between)


def test_a_seen_set_of_any_multiple_of_64_slots_every_slot_reachable_and_evenly_loaded(tmp_path):
    """kmc_slot_of / kmc_slot_next (csrc/kmc_common.h): the home slot of a fingerprint in a table of ANY multiple of 64 slots — what
    lets the 6.45 G-state stretch use 192 GiB instead of the 128 GiB power of two — compiled for the host: always below the
    capacity, the low six bits are the fingerprint's, the 64-slot groups are hit evenly (also by the fingerprints ONE shard owns:
    the owner is chosen by other bits), and the chain wraps at the capacity."""
    import subprocess
    src = tmp_path / "slot.cpp"
    src.write_text(r'''
#define KMC_HOST_EMU 1
#include "kmc_common.h"
#include <cstdio>
#include <vector>
int main() {
    const unsigned long long caps[] = {1024ull, 1088ull, 1ull << 20, 12500000000ull / 64 * 64, 1ull << 34, (1ull << 38) - 64};
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (unsigned long long cap : caps) {
        const unsigned long long groups = cap >> 6, buckets = groups < 997 ? groups : 997;
        std::vector<unsigned long long> hist(buckets, 0), hist_shard(buckets, 0);
        unsigned long long n_shard = 0;
        for (int k = 0; k < 2000000; ++k) {
            x = kmc_mix64(x + 0x9E3779B97F4A7C15ull);
            const unsigned long long fp = x ? x : 1, i = kmc_slot_of(fp, cap);
            if (i >= cap || (i & 63) != (fp & 63)) { printf("BAD slot %llu of %llu\n", i, cap); return 1; }
            hist[(unsigned long long)((__uint128_t)(i >> 6) * buckets / groups)]++;
            if (kmc_owner(fp, 8) == 3) { hist_shard[(unsigned long long)((__uint128_t)(i >> 6) * buckets / groups)]++; ++n_shard; }
        }
        for (unsigned long long b = 0; b < buckets; ++b) {
            const double want = 2000000.0 / buckets, got = (double)hist[b], wants = (double)n_shard / buckets, gots = (double)hist_shard[b];
            if (got < 0.8 * want || got > 1.2 * want || gots < 0.6 * wants || gots > 1.4 * wants) {
                printf("UNEVEN cap %llu bucket %llu: %.0f of %.0f, shard 3 of 8: %.0f of %.0f\n", cap, b, got, want, gots, wants);
                return 1;
            }
        }
        if (kmc_slot_next(cap - 1, cap) != 0 || kmc_slot_next(5, cap) != 6) { printf("BAD wrap\n"); return 1; }
    }
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "slot"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "kafka_specification_amd", "csrc"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
