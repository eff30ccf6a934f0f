"""CPU: the C-ABI library loads and exports every symbol include/polar_hip.h declares (no compute calls
without a GPU), argument validation, host-side helpers, and the N > 1 path under gloo with world_size 2."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO


def _lib():
    import polardecoding_amd as pa
    if not os.path.exists(pa.lib_path()):
        import __graft_entry__ as g
        g.build()
    return pa.load_library()


def test_every_declared_symbol_is_exported():
    lib = _lib()
    hdr = open(os.path.join(REPO, "include", "polar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(polar_[a-z_0-9]+)\s*\(", hdr)))
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in polar_hip.h but not exported"


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_product_library_exports_the_c_abi_and_nothing_else():
    """libpolar_hip.so exports exactly the polar_* functions include/polar_hip.h declares: no test-only entry point
    (polar_testing_*, the math probe, the four-per-wave kernel live in libpolar_hip_testing.so), no C++ symbol."""
    import polardecoding_amd as pa
    _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "polar_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(polar_[a-z_0-9]+)\s*\(", hdr)))
    assert _exported(pa.lib_path()) == declared
    assert not [s for s in _exported(pa.lib_path()) if "testing" in s]
    thdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "polar_hip_testing.h")).read(), flags=re.S)
    tdecl = sorted(set(re.findall(r"\b(polar_testing_[a-z_0-9]+)\s*\(", thdr)))
    assert len(tdecl) == 7
    assert _exported(pa.lib_path(testing=True)) == sorted(declared + tdecl)


def test_version_and_strerror():
    lib = _lib()
    assert b"gfx950" in lib.polar_version()
    assert lib.polar_strerror(0) == b"ok"
    assert b"invalid" in lib.polar_strerror(-1)


def test_create_rejects_bad_configs_before_touching_a_device():
    import polardecoding_amd as pa
    _lib()
    with pytest.raises(pa.PolarError):
        pa.Decoder(1000, 512, pa.ALGO_SCL, L=8)        # N not a power of two
    with pytest.raises(pa.PolarError):
        pa.Decoder(1024, 512, pa.ALGO_SCL, L=3)        # L not a power of two
    with pytest.raises(pa.PolarError):
        pa.Decoder(1024, 2000, pa.ALGO_SCL, L=8)       # K > N
    with pytest.raises(pa.PolarError):
        pa.Decoder(1024, 512, pa.ALGO_CASCL, L=8)      # CA-SCL without CRC taps
    with pytest.raises(pa.PolarError):
        pa.Decoder(1024, 512, pa.ALGO_CASCL, L=8, crc_taps=(1, 5, 6))  # g(D) without D^0


def test_no_cpu_fallback_in_product_package():
    """The product path must not import or call the oracle."""
    pkg = os.path.join(REPO, "polardecoding_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".c", ".cpp")):
                text = open(os.path.join(root, f), errors="replace").read()
                assert "oracle_py" not in text and "polar_oracle" not in text, f


def test_q_sequence_matches_oracle_table(oracle):
    import polardecoding_amd as pa
    assert pa.q_sequence(1024) == oracle.q_for(1024)
    assert pa.q_sequence(128) == oracle.q_for(128)


def test_frame_shard_partition():
    from polardecoding_amd.montecarlo import frame_shard
    for total in (0, 1, 7, 1 << 20, 12345):
        for world in (1, 2, 3, 8):
            spans = [frame_shard(total, r, world) for r in range(world)]
            assert sum(c for _, c in spans) == total
            pos = 0
            for s, c in spans:
                assert s == pos
                pos += c


def test_sequential_stop_cut():
    from polardecoding_amd.montecarlo import sequential_stop_cut
    fe = [0, 3, 0, 0, 1, 0, 2, 0]
    assert sequential_stop_cut(fe, 2) == (5, 2, 4)
    assert sequential_stop_cut(fe, 3) == (7, 3, 6)
    assert sequential_stop_cut(fe, 4) is None


WORKER = r"""
import os, sys
sys.path.insert(0, {repo!r})
import numpy as np, torch, torch.distributed as dist
from oracle import oracle_py as O            # checker standing in for the GPU decoder in this CPU test
from polardecoding_amd.montecarlo import fer_point, frame_shard, sequential_stop_cut_sharded
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
code = O.Code(128, 64, O.CRC6_TAPS)
sig = O.sigma_from_db(1.5)
us, ys = O.Sim(77).frames(code, sig, 96)     # every rank draws the same frame list and decodes only its shard
def dec(start, count):
    blk = bits = 0
    for i in range(start, start + count):
        uh, _, _ = O.decode(code, O.llr_from_y(ys[i], sig), "CASCL", L=8)
        e = O.count_bit_errors(code, us[i], uh)
        blk += e > 0; bits += e
    return blk, bits
res = fer_point(dec, 96, rank, world, dist)
# exact sequential stop rule over a sharded batch of 95 frames (uneven shards): per-frame error counts gathered in frame order
start, count = frame_shard(95, rank, world)
fe = []
for i in range(start, start + count):
    uh, _, _ = O.decode(code, O.llr_from_y(ys[i], sig), "CASCL", L=8)
    fe.append(O.count_bit_errors(code, us[i], uh))
cut = sequential_stop_cut_sharded(fe, 95, 5, rank, world, dist)
if rank == 0:
    print("RESULT", res[0], res[1], res[2])
print("CUT", rank, *(cut if cut else (-1, -1, -1)))
dist.destroy_process_group()
"""


def test_two_rank_gloo_matches_single_process(oracle, tmp_path):
    """world_size-2 gloo run of the sharded FER point == the single-process count over the same frames."""
    code = oracle.Code(128, 64, oracle.CRC6_TAPS)
    sig = oracle.sigma_from_db(1.5)
    us, ys = oracle.Sim(77).frames(code, sig, 96)
    blk = bits = 0
    for i in range(96):
        uh, _, _ = oracle.decode(code, oracle.llr_from_y(ys[i], sig), "CASCL", L=8)
        e = oracle.count_bit_errors(code, us[i], uh)
        blk += e > 0
        bits += e
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(repo=REPO))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-2000:]
    line = [l for l in outs[0][0].splitlines() if l.startswith("RESULT")][0].split()
    assert [int(x) for x in line[1:]] == [blk, bits, 96]
    # the cut at the 5th block error, as one process sees it
    from polardecoding_amd.montecarlo import sequential_stop_cut
    fe = []
    for i in range(95):
        uh, _, _ = oracle.decode(code, oracle.llr_from_y(ys[i], sig), "CASCL", L=8)
        fe.append(oracle.count_bit_errors(code, us[i], uh))
    want = sequential_stop_cut(fe, 5)
    assert want is not None
    for o, _ in outs:
        cl = [l for l in o.splitlines() if l.startswith("CUT")][0].split()
        assert tuple(int(x) for x in cl[2:]) == want


def test_bench_launches_its_own_ranks_under_gloo():
    """`python bench.py --gpus 2` with no launcher around it: the parent (which never touches a GPU) starts two ranks
    through torch.distributed.run and relays rank 0's JSON line.  CPU rehearsal of that control path: gloo instead of
    RCCL, nothing decoded (--rehearse-cpu), same barriers and reductions."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--rehearse-cpu"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["steps"] == 3 and d["rehearsal"] is True
    assert d["counter_sum"] == [3, 30]          # (1 + 2, 10 + 20): the SUM all-reduce over both ranks
    assert d["value"] is None                   # a rehearsal measures nothing
    # what the N-rank line says about the collective backend: the number of ranks an all-reduce of ones really summed
    # over, and every rank's device name gathered through the same backend
    assert d["rccl_ranks"] == 2 and len(d["devices"]) == 2 and "rank 1" in d["devices"][1]
    assert d["config"]["name"] == "cascl_1024_l8" and d["config"]["frames_per_gpu_per_step"] == 1 << 17
    # BASELINE config 5 has an N-rank line of its own: --config cascl_4096_l32, 2^15 frames per GPU (2^18 over 8)
    out5 = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--rehearse-cpu",
                           "--config", "cascl_4096_l32"], capture_output=True, text=True, timeout=600, env=env)
    assert out5.returncode == 0, out5.stderr[-3000:]
    d5 = json.loads([l for l in out5.stdout.splitlines() if l.startswith("{")][0])
    assert d5["n_gpus"] == 2 and d5["rccl_ranks"] == 2 and "N=4096 K=2048 CA-SCL L=32" in d5["metric"]
    assert d5["config"]["name"] == "cascl_4096_l32" and d5["config"]["frames_per_gpu_per_step"] == 1 << 15
    # a launcher that started a different number of ranks than --gpus says is an error, not a silent n_gpus = 1
    bad = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4", "--rehearse-cpu"],
                         capture_output=True, text=True, timeout=120, env=dict(env, WORLD_SIZE="2", RANK="0"))
    assert bad.returncode != 0 and "WORLD_SIZE=2" in bad.stderr
    # an EXTERNAL launcher (torchrun started by somebody else, not bench.py's own launch()) gets the dmabuf-IPC setting RCCL
    # needs on this image too: run() puts it into the environment before torch is imported
    src = open(os.path.join(REPO, "bench.py")).read()
    body = src[src.index("def run(args):"):]
    assert body.index('os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")') < body.index("import torch")


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: what the timed path returned, as float64 .npy, exact, within the byte budget; a larger output
    is cut to the same seeded sample of frames every time.  --steps 0 is refused (it must be the number of timed steps)."""
    import bench
    rng = np.random.default_rng(1)
    words = rng.integers(-2 ** 31, 2 ** 31, size=(1000, 32), dtype=np.int64).astype(np.int32)
    rows = bench.dump_outputs(str(tmp_path / "all"), {"out_bits": words})
    got = np.load(tmp_path / "all" / "out_bits.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.int32), words) and len(rows) == 1000
    assert np.array_equal(np.load(tmp_path / "all" / "frame_index.npy"), np.arange(1000))
    budget = 100 * 33 * 8 + 2 * 128                # room for 100 frames of 32 words plus their index, and two headers
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"out_bits": words}, budget=budget)
    idx = np.load(tmp_path / "a" / "frame_index.npy").astype(np.int64)
    assert len(idx) == 100 and (np.diff(idx) > 0).all()
    assert np.array_equal(np.load(tmp_path / "a" / "out_bits.npy").astype(np.int32), words[idx])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= budget
    for f in ("frame_index.npy", "out_bits.npy"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--rehearse-cpu"] + bad,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "--steps must be >= 1" in out.stderr


def test_fn_matrix_file_format(tmp_path):
    """The N x N 0/1 matrix the reference reads from stdin (SCL_1024.c:207-217): written, read back the reference's way,
    recognised as the Kronecker power; a damaged copy is counted and rejected; its rows ARE the butterfly encoder."""
    from polardecoding_amd import fnfile
    p = tmp_path / "Fn_128.txt"
    fnfile.write_fn(str(p), 128)
    m, illegal = fnfile.read_fn(str(p))
    assert m.shape == (128, 128) and illegal == 0 and fnfile.is_kronecker(m)
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2, 128)
    x = (u @ m) % 2                                   # x = u Fn, SCL_1024.c:242-250
    y = u.copy()
    s = 1
    while s < 128:                                     # the butterfly form used by the harness and the generator kernel
        for j in range(128):
            if not (j & s):
                y[j] ^= y[j + s]
        s *= 2
    assert np.array_equal(x, y)
    txt = p.read_text().split()
    txt[5] = "7"
    txt[300] = "1" if txt[300] == "0" else "0"
    q = tmp_path / "bad.txt"
    q.write_text(" ".join(txt))
    m2, illegal2 = fnfile.read_fn(str(q), 128)
    assert illegal2 == 1 and not fnfile.is_kronecker(m2)


def test_crc_matrix_file_loader_of_the_c_abi(tmp_path):
    """polar_crc_matrix_load / _save (csrc/crc_matrix.hip): the reference's CRC_6.dat -- UTF-16LE, BOM, CRLF, 64 x 6 --
    gives g(D) = D^6 + D^5 + 1 and the matrix the Python reader sees; the Gc[K][r] literal layout of
    CASCL_1024_sys.c:48-561 (braces, commas, ASCII) loads as CRC-24C; anything that is not D^(r+i) mod g is refused."""
    import polardecoding_amd as pa
    from polardecoding_amd import crcfile
    _lib()
    golden = os.path.join(REPO, "tests", "golden", "CRC_6.dat")
    taps, m = pa.load_crc_matrix(golden)
    assert taps == (0, 5, 6) and m.shape == (64, 6)
    assert np.array_equal(m, crcfile.load(golden))
    assert np.array_equal(m, crcfile.systematic_parity_matrix(64, (0, 5, 6)))
    out = tmp_path / "c6.dat"
    pa.save_crc_matrix(str(out), 64, (0, 5, 6))
    assert out.read_bytes() == open(golden, "rb").read()          # byte for byte the reference's file
    # the layout of the C literal: `{1, 1, 1, 0, ...},` per row, plain ASCII
    m24 = crcfile.systematic_parity_matrix(512, pa.CRC24C_TAPS)
    lit = tmp_path / "gc.txt"
    lit.write_text("{\n" + ",\n".join("{" + ", ".join(str(int(v)) for v in row) + "}" for row in m24) + "\n};\n")
    taps24, back = pa.load_crc_matrix(str(lit))
    assert taps24 == tuple(pa.CRC24C_TAPS) and np.array_equal(back, m24)
    # refusals
    def refuse(mat_bytes):
        p = tmp_path / "bad.dat"
        p.write_bytes(mat_bytes)
        with pytest.raises(pa.PolarError):
            pa.load_crc_matrix(str(p))
    bad = m.copy(); bad[17, 2] ^= 1
    refuse(crcfile.dumps(bad))                                    # one entry flipped: row 17 is not D^23 mod g
    refuse(crcfile.dumps(m[:, :5]))                               # a column missing: rows no longer follow from row 0
    refuse(crcfile.dumps(m).replace("1 0 0 0 0 1".encode("utf-16-le"), "1 0 0 0 0 2".encode("utf-16-le"), 1))   # not 0/1
    refuse(b"1 0 0 0 0 1\n1 1 0 0 0\n")                         # ragged
    refuse(b"0 1 0 0 0 1\n")                                     # g(D) without D^0
    refuse(b"")                                                   # empty
    refuse(b"\xff\xfe1")                                        # odd number of bytes behind the BOM
    with pytest.raises(pa.PolarError):
        pa.load_crc_matrix(str(tmp_path / "does_not_exist.dat"))
    # a prefix of the rows is a valid (shorter) matrix: K = 32 payload bits
    short = tmp_path / "c6_32.dat"
    short.write_bytes(crcfile.dumps(m[:32]))
    taps32, m32 = pa.load_crc_matrix(str(short))
    assert taps32 == (0, 5, 6) and m32.shape == (32, 6)


def test_register_budget_of_the_tuned_kernels(tmp_path):
    """Register allocation decides these kernels' speed more than any source change of round 3 did: seven spilled VGPRs in
    k_scl_big's chain() cost 8 %, thirty-seven more in k_scl_fast2 cost 9 % (4.0).  The budgets the measured
    binaries had are pinned here (hipcc cross-compiles without a GPU): BASELINE config 5's kernel must stay within the few spilled VGPRs of the measured binary at three
    wavefronts per SIMD, the headline kernel must stay within its three-wavefront budget with no more spills than measured."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    import __graft_entry__ as g
    want = {
        # split 4 / 7 / 1 + chain() (the shipped kernel of BASELINE config 5): measured with 2 spilled VGPRs; the same kernel with 50
        # (per-element mask constants hoisted out of the leaf loop and reloaded one by one) lost 30 %; 7 in chain() lost 8 %
        "k_big_f64": [("_ZN5polar9k_scl_bigIddLi5ELi4ELi7ELi1ELi1EEEvNS_9SclParamsE", 168, 4),
                      ("_ZN5polar9k_scl_bigIddLi5ELi3ELi7ELi1ELi0EEEvNS_9SclParamsE", 128, 0)],   # N = 1024, L = 32: four wavefronts per SIMD
        "k_fast2": [("_ZN5polar11k_scl_fast2IddLb1EEEvNS_9SclParamsE", 168, 60),
                    ("_ZN5polar11k_scl_fast2IddLb0EEEvNS_9SclParamsE", 168, 60)],
    }
    for tu, kernels in want.items():
        out = tmp_path / (tu + ".s")
        subprocess.check_call([hipcc] + g.HIPCC_FLAGS + ["-S", "--cuda-device-only", "-o", str(out),
                                                         os.path.join(g.CSRC, tu + ".hip")],
                              cwd=g.CSRC, stderr=subprocess.DEVNULL)
        txt = out.read_text()
        for name, max_vgpr, max_spill in kernels:
            m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt)
            assert m, name
            assert int(m.group(1)) <= max_vgpr and int(m.group(2)) <= max_spill, (name, m.group(1), m.group(2))
