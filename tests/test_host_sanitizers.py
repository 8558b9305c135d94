"""CPU: the host half of the product (format builders, team scheduler, planner, ingest) compiled with
AddressSanitizer + UBSan and driven by tests/host_asan.cpp, and the engines' operand layer (csrc/operand_view.h) over host stand-ins for the device ABI, driven by
tests/host_operand_view.cpp, and the two engines with the owners of their device resources (csrc/dev_owned.h) over such stand-ins, driven by
tests/host_engine_resources.cpp, and the row engine's cross-stream ORDER on a split engine, replayed with vector clocks from the stand-ins' log by
tests/host_engine_streams.cpp (GPU sanitizers are not available on the pool)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_host_code_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "crp-spmm_amd", "csrc")
    files = [os.path.join(src, f) for f in ("panel_format.cpp", "panel_order.cpp", "team_format.cpp", "team_cluster.cpp", "team2_format.cpp", "team2r_format.cpp", "team_order.cpp", "locality.cpp", "spmat_part.cpp", "mmio_utils.cpp", "host_support.cpp", "knobs.cpp", "dispatch.cpp")]
    exe = str(tmp_path / "host_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + src,
           os.path.join(ROOT, "tests", "host_asan.cpp"), *files, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", CRPSPMM_NUM_THREADS="4", CRPSPMM_SYNC_RELEASE="1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "HOST_ASAN_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_operand_view_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_operand_view")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "crp-spmm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host_operand_view.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0 and "HOST_OPERAND_VIEW_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_engine_resources_under_asan_ubsan(tmp_path):
    """Every device block, stream, event and matrix handle the engines create is released exactly once by crp_*_spmm_free, a plan-only
    engine touches no device function, and the owners release what they hold once (tests/host_engine_resources.cpp)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "crp-spmm_amd", "csrc")
    files = [os.path.join(src, f) for f in ("rp_engine.cpp", "rp_attention.cpp", "rp_gat.cpp", "para2d_engine.cpp", "knobs.cpp", "host_support.cpp")]
    exe = str(tmp_path / "host_engine_resources")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + src,
           os.path.join(ROOT, "tests", "host_engine_resources.cpp"), *files, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "HOST_ENGINE_RESOURCES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    t = subprocess.run([exe, "--trace"], capture_output=True, text=True, timeout=600, env=env)
    names = t.stdout.split()
    assert t.returncode == 0 and len(names) > 1000 and "dev_free(null)" not in names and "csr_dev_destroy(null)" not in names


def test_engine_stream_order_under_asan_ubsan(tmp_path):
    """The split row engine (a fake communicator of 2 ranks) orders every conflicting pair of device accesses across the caller's
    stream, its own stream and the exchange stream -- exec, exec_t, sddmm, attention, attention_bwd, the GAT and GATv2 forward (csrc/rp_gat.cpp: two
    packs and two exchanges beside the interior kernel, and the narrow buffers set up again for another number of heads),
    update_values and update_values_dev, on two caller streams -- and the same checker reports a race once one stream_wait_event
    is taken out of the log, for a GAT call on the narrow receive buffer among others; the same call list with the phases timed is
    ordered too, every exchange on a caller's stream (tests/host_engine_streams.cpp; its --dump prints both logs for diff)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "crp-spmm_amd", "csrc")
    files = [os.path.join(src, f) for f in ("rp_engine.cpp", "rp_attention.cpp", "rp_gat.cpp", "knobs.cpp", "host_support.cpp")]
    exe = str(tmp_path / "host_engine_streams")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + src,
           os.path.join(ROOT, "tests", "host_engine_streams.cpp"), *files, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "HOST_ENGINE_STREAMS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    stats = dict(kv.split("=") for kv in r.stdout.split()[1:])
    assert int(stats["streams"]) >= 4 and int(stats["exchanges"]) > 0 and int(stats["needed"]) > 0 and int(stats["control_races"]) > 0, r.stdout
    assert int(stats["gat_exchanges"]) > 0 and int(stats["gat_cross_stream_waits"]) > 0 and int(stats["gat_control_races"]) > 0, r.stdout
