"""Retuning a channel of a running front end, the parts that need no GPU:

  a. the device code objects of the built libhfdl_gpu.so: as many as there are kernel files, each with its static symbol table, the
     three retune kernels among their kernel descriptors.  (The first attempt at this feature died in the host process at the first
     launch of a kernel of a NEW code object that had been linked without .symtab to fit the library's size cap: the runtime's loader
     walks .symtab unless told otherwise, and a code object is loaded at the first launch of one of its kernels.);
  b. the entry point is exported;
  c. the host library's path -- hfdl_frontend_retune / hfdl_frontend_schedule_retune, the front-end thread's retune_step, hfdl_replay
     --retune -- under the address and undefined-behaviour sanitizers as a stand-alone program against tests/hostsim/gpu_standin_retune.c;
  d. planner.h FftOrder with the retune transition, over every short call sequence (tests/hostsim/retune_order_check.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dumphfdl_amd")
HOST = os.path.join(PKG, "host")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
KERNEL_FILES = 4              # KERNEL_OBJS of dumphfdl_amd/csrc/objects.sh: fft, fold, demod, spectrum -- what the parent had
RETUNE_KERNELS = ("retune_channelizer_kernel", "retune_demod_kernel", "retune_freq_kernel")
BLOCK = 3072                  # the stand-in's geometry.input_size
NBLOCKS = 67
FS = 250000
TIMEOUT = 30


def tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.fail("%s is missing: the code objects cannot be looked at" % path)
    return path


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    """[(sections, symbols)] of every gfx950 code object in libhfdl_gpu.so: .hip_fatbin dumped, cut at the bundle magic, unbundled"""
    lib = os.path.join(PKG, "libhfdl_gpu.so")
    if not os.path.exists(lib):
        pytest.fail("libhfdl_gpu.so is not built")
    d = tmp_path_factory.mktemp("co")
    fatbin = str(d / "fatbin")
    subprocess.check_call([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, lib, str(d / "unused.so")])
    data = open(fatbin, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = []
    at = data.find(magic)
    while at >= 0:
        starts.append(at)
        at = data.find(magic, at + 1)
    out = []
    for i, s in enumerate(starts):
        piece = str(d / ("bundle%d" % i))
        with open(piece, "wb") as f:
            f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        targets = subprocess.check_output([tool("clang-offload-bundler"), "--list", "--type=o", "--input=" + piece], text=True).split()
        gfx = [t for t in targets if "gfx950" in t]
        assert len(gfx) == 1 and all("gfx950" in t or t.startswith("host-") for t in targets), targets
        co = piece + ".co"
        subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + piece, "--targets=" + gfx[0], "--output=" + co])
        sections = subprocess.check_output([tool("llvm-readelf"), "-S", co], text=True)
        symbols = subprocess.check_output([tool("llvm-readelf"), "-s", "--wide", co], text=True)
        out.append((sections, symbols))
    return out


def test_every_code_object_keeps_its_symbol_table(code_objects):
    assert len(code_objects) == KERNEL_FILES
    for sections, _ in code_objects:
        names = [ln.split("]")[1].split()[0] for ln in sections.splitlines() if ln.lstrip().startswith("[") and "]" in ln and len(ln.split("]")[1].split()) > 1]
        assert ".symtab" in names and ".strtab" in names and ".dynsym" in names, names


def test_the_retune_kernels_are_in_existing_code_objects(code_objects):
    def kd_in_symtab(symbols, kernel):
        table = symbols.split("Symbol table '.symtab'")[1]
        return any(kernel in ln and ln.rstrip().endswith(".kd") for ln in table.splitlines())
    homes = {k: [i for i, (_, symbols) in enumerate(code_objects) if kd_in_symtab(symbols, k)] for k in RETUNE_KERNELS}
    assert all(len(h) == 1 for h in homes.values()), homes
    # beside the kernels that own what they write: the forward FFT's riders, the demodulator and the burst decoder
    for k, other in zip(RETUNE_KERNELS, ("fft_rpass3", "demod_kernel", "burst_decode_kernel")):
        assert other in code_objects[homes[k][0]][1], (k, other)


def test_entry_point_is_exported():
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "libhfdl_gpu.so")], text=True)
    assert any(ln.split()[-1] == "hfdl_gpu_frontend_retune_channel" and ln.split()[-2] == "T" for ln in syms.splitlines())


def test_host_prototypes_by_type():
    """tests/abi/hfdl_host_retune_abi.c: the two prototypes include/hfdl_host.h adds, in C11 with every warning an error"""
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi", "hfdl_host_retune_abi.c")])


# ---------------------------------------------------------------- c. the host thread against the stand-in

def build_replay(d, standin):
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    exe = str(d / ("hfdl_replay_" + standin))
    subprocess.check_call(["gcc", "-g", "-O1", "-std=c11", "-D_GNU_SOURCE"] + san + ["-I", os.path.join(ROOT, "include"), "-I", HOST] +
                          [os.path.join(HOST, f) for f in ("hfdl_replay.c", "ring.c", "blocks.c", "input.c", "sink.c", "frontend.c")] +
                          [os.path.join(ROOT, "tests", "hostsim", standin + ".c"), "-o", exe, "-lpthread", "-lm"])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("retune")
    probe = d / "p.c"
    probe.write_text("int main(void){return 0;}\n")
    if subprocess.run(["gcc", "-fsanitize=address,undefined", str(probe), "-o", str(d / "p")], capture_output=True).returncode != 0:
        pytest.fail("this gcc has no sanitizer runtime: the host thread's retune path cannot be run under the sanitizers")
    return build_replay(d, "gpu_standin_retune"), build_replay(d, "gpu_standin")


def fnv1a64(blocks):
    h = np.full(len(blocks), 0xcbf29ce484222325, np.uint64)
    prime = np.uint64(0x100000001b3)
    for column in blocks.T.astype(np.uint64):
        h = (h ^ column) * prime
    return [int(x) for x in h]


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    raw = np.random.default_rng(29).integers(0, 256, (NBLOCKS * BLOCK + 777) * 4, dtype=np.uint8)
    path = tmp_path_factory.mktemp("iq") / "in.cs16"
    raw.tofile(path)
    return str(path), fnv1a64(raw[:NBLOCKS * BLOCK * 4].reshape(NBLOCKS, BLOCK * 4))


def run(exe, source, *options, **standin):
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.update({"HFDL_STANDIN_" + k.upper(): str(v) for k, v in standin.items()})
    cmd = [exe, "--iq-file", source, "--sample-rate", str(FS), "--sample-format", "CS16", "--read-buffer-size", "4096",
           "--centerfreq", "10000"] + list(options) + ["10010", "10020"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT, env=env)


def clean(stderr):
    return "Sanitizer" not in stderr and "runtime error" not in stderr and "gpu stand-in:" not in stderr


def pdus_of(stdout):
    """(frequency, block number, hash) of every printed PDU, in the order printed"""
    got = []
    for line in stdout.splitlines():
        assert line.startswith("PDU freq=") and " len=16 " in line, line
        octets = bytes.fromhex(line.split()[-1])
        got.append((int(line.split()[1][5:]), int.from_bytes(octets[:8], "little"), int.from_bytes(octets[8:], "little")))
    return got


def at_block(k):
    """a time that lies behind the first sample of block k - 1 and not behind that of block k"""
    return "%.6f" % ((k - 0.5) * BLOCK / FS)


KNOBS = [dict(), dict(prefetch=17, copy_lag=3)]


def statsd_a2(stderr):
    """{frequency: A2_found total} of hfdl_replay --statsd-print"""
    return {int(ln.split()[2]): int(ln.split("A2_found=")[1].split()[0]) for ln in stderr.splitlines() if ln.startswith("STATSD counter ")}


@pytest.mark.parametrize("knobs", KNOBS)
def test_the_boundary_is_the_block(programs, recording, knobs):
    """The rule "a PDU keeps the frequency of the moment its block was pushed" is the stand-in's own model here (gpu_standin_retune.c);
    what this checks of frontend.c is that retune_step() runs between the push of block k - 1 and the push of block k -- blocks uploaded
    ahead included -- and that nothing is lost, repeated or reordered around it."""
    path, hashes = recording
    k = 30
    assert 0 < k < NBLOCKS
    out = run(programs[0], path, "--retune", at_block(k) + ":10010:10030", **knobs)
    assert out.returncode == 0 and clean(out.stderr) and out.stderr == "", out.stderr[-2000:]
    assert pdus_of(out.stdout) == [(10010000 if b < k else 10030000, b, h) for b, h in enumerate(hashes)]


@pytest.mark.parametrize("knobs", KNOBS)
def test_two_chained_requests(programs, recording, knobs, tmp_path):
    path, hashes = recording
    k1, k2 = 9, 41
    count = tmp_path / "calls"
    out = run(programs[0], path, "--retune", at_block(k1) + ":10010:10030", "--retune", at_block(k2) + ":10030:10040",
              retune_count=count, **knobs)
    assert out.returncode == 0 and clean(out.stderr) and out.stderr == "", out.stderr[-2000:]
    assert pdus_of(out.stdout) == [(10010000 if b < k1 else 10030000 if b < k2 else 10040000, b, h) for b, h in enumerate(hashes)]
    assert count.read_text().strip() == "2"
    # both at one boundary: a -> b and b -> c queued back to back
    out = run(programs[0], path, "--retune", at_block(k1) + ":10010:10030", "--retune", at_block(k1) + ":10030:10040", **knobs)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    assert pdus_of(out.stdout) == [(10010000 if b < k1 else 10040000, b, h) for b, h in enumerate(hashes)]


@pytest.mark.parametrize("knobs", KNOBS)
def test_refusals_are_named_once_and_the_stream_goes_on(programs, recording, knobs, tmp_path):
    path, hashes = recording
    whole = [(10010000, b, h) for b, h in enumerate(hashes)]
    # nobody listens on 10099 kHz; 10020 kHz is taken
    for req in ("10099:10030", "10010:10020"):
        out = run(programs[0], path, "--retune", at_block(12) + ":" + req, **knobs)
        assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
        assert out.stderr.count("retune ") == 1 and "refused" in out.stderr and pdus_of(out.stdout) == whole
    # the device refuses the first of two: named once with its text, the second is applied (to channel 1: no PDU changes)
    count = tmp_path / "calls"
    text = "injected: the device says no"
    out = run(programs[0], path, "--retune", at_block(12) + ":10010:10030", "--retune", at_block(20) + ":10020:10050", "--bench",
              fail_retune=1, fail_text=text, retune_count=count, **knobs)
    assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
    assert out.stderr == "retune 10010000 -> 10030000 Hz refused: " + text + "\n"
    rs = json.loads(out.stdout)
    assert (rs["blocks"], rs["pdus"], rs["retunes"]) == (NBLOCKS, NBLOCKS, 1) and count.read_text().strip() == "2"
    out = run(programs[0], path, "--retune", at_block(12) + ":10010:10030", fail_retune=1, fail_text=text, **knobs)
    assert out.returncode == 0 and clean(out.stderr) and pdus_of(out.stdout) == whole


@pytest.mark.parametrize("knobs", KNOBS)
def test_counters_follow_the_frequency_and_never_run_backwards(programs, recording, knobs):
    """The stand-in counts one A2 detection per pushed block on channel 0.  With statistics that are a fresh channel's from the call on
    (what the library gives), every event is published once: the k blocks before the boundary under the old frequency (the thread
    publishes before it retunes), the rest under the new.  With statistics that LAG the retune by three blocks -- the old counter
    still showing, then dropping; requests for the other channel one and five blocks later make the thread publish inside the lag
    and after it -- the old frequency's total is the same, the new one's holds every later event and the lagging reads on top, and
    the run ends: a counter found below the snapshot is counted from zero, not "up" through 2^32."""
    path, _ = recording
    k = 30
    out = run(programs[0], path, "--statsd-print", "--retune", at_block(k) + ":10010:10030", **knobs)
    assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
    assert statsd_a2(out.stderr) == {10010000: k, 10030000: NBLOCKS - k}
    lag = 3
    out = run(programs[0], path, "--statsd-print", "--retune", at_block(k) + ":10010:10030", "--retune", at_block(k + 1) + ":10020:10050",
              "--retune", at_block(k + 5) + ":10050:10060", stats_lag=lag, **knobs)
    assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
    got = statsd_a2(out.stderr)
    # the publish at block k + 1 reads the old counter (k + 1, or up to k + lag in later timed publishes) against the zeroed snapshot;
    # the one at block k + 5 finds 5 below it: counted from zero
    assert got[10010000] == k and NBLOCKS - k + (k + 1) <= got[10030000] <= NBLOCKS - k + (k + lag), got


def test_bench_reports_retunes(programs, recording):
    out = run(programs[0], recording[0], "--retune", at_block(3) + ":10010:10030", "--retune", at_block(50) + ":10020:10050", "--bench", prefetch=17, copy_lag=3)
    assert out.returncode == 0 and clean(out.stderr) and out.stderr == "", out.stderr[-2000:]
    rs = json.loads(out.stdout)
    assert (rs["blocks"], rs["pdus"], rs["retunes"]) == (NBLOCKS, NBLOCKS, 2)
    out = run(programs[0], recording[0], "--bench")
    assert json.loads(out.stdout)["retunes"] == 0


def test_a_library_without_the_entry_point_refuses_cleanly(programs, recording):
    """linked with the plain stand-in the weak symbol is null"""
    path, hashes = recording
    out = run(programs[1], path, "--retune", at_block(30) + ":10010:10030", prefetch=17, copy_lag=3)
    assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
    assert out.stderr == "retune 10010000 -> 10030000 Hz refused: this GPU library cannot retune\n"
    assert pdus_of(out.stdout) == [(10010000, b, h) for b, h in enumerate(hashes)]


def test_bad_option_text(programs, recording):
    for bad in ("1:10010", "x:10010:10030", "-1:10010:10030", "1:10010:10030:7"):
        out = run(programs[0], recording[0], "--retune", bad)
        assert out.returncode == 1 and "--retune wants" in out.stderr and out.stdout == ""


def test_an_exported_channel_starts_a_new_file(programs, recording, tmp_path):
    """the retuned channel's samples up to the boundary are in <old>.cf32, the rest in <new>.cf32; the other channel's file is whole"""
    path, _ = recording
    k = 30
    out = run(programs[0], path, "--iq-export-dir", str(tmp_path), "--retune", at_block(k) + ":10010:10030", prefetch=17, copy_lag=3)
    assert out.returncode == 0 and clean(out.stderr) and out.stderr == "", out.stderr[-2000:]
    count = lambda b, s: 1 + (b * 7 + s * 3) % 6                      # the stand-in's export_count()
    sizes = {f: os.path.getsize(tmp_path / f) // 8 for f in os.listdir(tmp_path)}
    assert sizes == {"10010000.cf32": sum(count(b, 0) for b in range(k)), "10030000.cf32": sum(count(b, 0) for b in range(k, NBLOCKS)),
                     "10020000.cf32": sum(count(b, 1) for b in range(NBLOCKS))}


# ---------------------------------------------------------------- d. the order of the forward FFTs around a retune

def test_fft_order_with_retunes_over_every_short_call_sequence(tmp_path):
    """tests/hostsim/retune_order_check.cpp: tests/hostsim/fft_order_check.cpp's model of the front end's launches and waits with a sixth
    call, the retune, in every sequence of up to seven calls: the retune's kernel is ordered behind every forward FFT queued before it
    wherever it ran, the next forward FFT on either stream behind the kernel, no stream waits for an event no launch carries, and
    nothing of what the sequences without a retune guarantee is lost."""
    exe = str(tmp_path / "retune_order_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "hostsim", "retune_order_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    assert int(out.stdout.split()[0]) > 1_000_000
