"""The host library's front-end thread (dumphfdl_amd/host/frontend.c) run on the CPU: hfdl_replay.c and the host sources linked with
tests/hostsim/gpu_standin.c instead of libhfdl_gpu.so, built with the address and undefined-behaviour sanitizers.  The stand-in reads a
queued block's memory only when its copy is first reported complete and puts the block's FNV-1a hash into the block's PDU, so a ring
slot given back to the producer too early shows as a wrong hash; its knobs (prefetch depth, copy lag, injected failures) are described
at the top of that file."""
import fcntl
import json
import math
import os
import select
import subprocess
import termios
import time
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dumphfdl_amd", "host")
BLOCK = 3072                  # the stand-in's geometry.input_size
OUT_PER_BLOCK = 6             # ... and max_outputs_per_block
PREFETCH_MAX = 17             # HFDL_GPU_PREFETCH_MAX
RING_BLOCKS = PREFETCH_MAX + 5        # block_connect_one2one() with the small read buffer used here
NBLOCKS = 3 * RING_BLOCKS + 1         # the file is several times the ring: a slot given back early is overwritten before it is hashed
FRAGMENT = 1234               # samples behind the last whole block
BPS = {"CS16": 4, "CU8": 2, "CF32": 8}
FS = 250000
LIVE_FS = 96000              # grace period 8 ms: the live case's pause of ten of them leaves a loaded host room
TIMEOUT = 30


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    d = tmp_path_factory.mktemp("fe")
    probe = d / "p.c"
    probe.write_text("int main(void){return 0;}\n")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(["gcc"] + san + [str(probe), "-o", str(d / "p")], capture_output=True).returncode != 0:
        pytest.skip("this gcc has no sanitizer runtime")
    exe = str(d / "hfdl_replay_standin")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=c11", "-D_GNU_SOURCE"] + san + ["-I", os.path.join(ROOT, "include"), "-I", HOST] +
                          [os.path.join(HOST, f) for f in ("hfdl_replay.c", "ring.c", "blocks.c", "input.c", "sink.c", "frontend.c")] +
                          [os.path.join(ROOT, "tests", "hostsim", "gpu_standin.c"), "-o", exe, "-lpthread", "-lm"])
    return exe


@pytest.fixture(scope="module")
def wrap_check(replay):
    """tests/hostsim/frontend_wrap_check.c: the thread in front of a ring that is no whole number of blocks long"""
    exe = os.path.join(os.path.dirname(replay), "frontend_wrap_check")
    subprocess.check_call(["gcc", "-g", "-O1", "-std=c11", "-D_GNU_SOURCE", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", HOST] +
                          [os.path.join(HOST, f) for f in ("ring.c", "blocks.c", "input.c", "sink.c", "frontend.c")] +
                          [os.path.join(ROOT, "tests", "hostsim", f) for f in ("frontend_wrap_check.c", "gpu_standin.c")] + ["-o", exe, "-lpthread", "-lm"])
    return exe


def fnv1a64(blocks):
    """FNV-1a 64 of every row of a 2-D uint8 array"""
    h = np.full(len(blocks), 0xcbf29ce484222325, np.uint64)
    prime = np.uint64(0x100000001b3)
    for column in blocks.T.astype(np.uint64):
        h = (h ^ column) * prime
    return [int(x) for x in h]


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """one random file per sample format and the hash of each of its whole blocks"""
    d = tmp_path_factory.mktemp("iq")
    rng = np.random.default_rng(17)
    out = {}
    for fmt, bps in BPS.items():
        raw = rng.integers(0, 256, (NBLOCKS * BLOCK + FRAGMENT) * bps, dtype=np.uint8)
        path = d / ("in." + fmt.lower())
        raw.tofile(path)
        out[fmt] = (str(path), raw, fnv1a64(raw[:NBLOCKS * BLOCK * bps].reshape(NBLOCKS, BLOCK * bps)))
    return out


def run(exe, source, fmt, *options, fs=FS, stdin=None, **standin):
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.update({"HFDL_STANDIN_" + k.upper(): str(v) for k, v in standin.items()})
    cmd = [exe, "--iq-file", source, "--sample-rate", str(fs), "--sample-format", fmt, "--read-buffer-size", "4096",
           "--centerfreq", "10000"] + list(options) + ["10010", "10020"]
    if stdin is not None:
        return subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT, env=env)


def clean(stderr):
    return "Sanitizer" not in stderr and "runtime error" not in stderr and "gpu stand-in:" not in stderr


def pdus_of(stdout):
    """(block number, hash) of every printed PDU, in the order printed"""
    got = []
    for line in stdout.splitlines():
        assert line.startswith("PDU freq=10010000 ") and " len=16 " in line, line
        octets = bytes.fromhex(line.split()[-1])
        got.append((int.from_bytes(octets[:8], "little"), int.from_bytes(octets[8:], "little")))
    return got


@pytest.mark.parametrize("fmt,depth,lag", [("CS16", 0, 0), ("CS16", 0, 3), ("CS16", PREFETCH_MAX, 0), ("CS16", PREFETCH_MAX, 3),
                                           ("CU8", PREFETCH_MAX, 3), ("CF32", PREFETCH_MAX, 3)])
def test_replay_delivers_every_block_once_and_right(replay, recordings, fmt, depth, lag):
    path, raw, hashes = recordings[fmt]
    out = run(replay, path, fmt, prefetch=depth, copy_lag=lag)
    assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
    assert pdus_of(out.stdout) == list(enumerate(hashes))
    loops = 3
    out = run(replay, path, fmt, "--loop", str(loops), "--bench", prefetch=depth, copy_lag=lag)
    assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
    rs = json.loads(out.stdout)
    blocks = loops * (len(raw) // BPS[fmt]) // BLOCK
    assert (rs["blocks"], rs["samples"], rs["pdus"]) == (blocks, blocks * BLOCK, blocks)
    assert (rs["block_samples"], rs["bytes_per_sample_over_pcie"], rs["channels"], rs["zero_copy_ring"]) == (BLOCK, BPS[fmt], 2, True)
    assert rs["lpdu_walk_on_device"] == {"mpdus": blocks, "lpdus": 2 * blocks, "good_fcs": blocks, "bad_fcs": blocks}


@pytest.mark.parametrize("depth,lag", [(0, 0), (PREFETCH_MAX, 3)])
def test_blocks_that_wrap_the_ring_go_through_the_bounce_copy(wrap_check, recordings, depth, lag):
    """A page-locked cf32 ring of seven blocks and a third: about every seventh block wraps around the end of the storage.  The
    thread gives the leased slots in front of it back first (waiting for their copies), then copies the block out; every block
    still arrives once, in order, with the file's bytes."""
    path, _, hashes = recordings["CF32"]
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", HFDL_STANDIN_PREFETCH=str(depth), HFDL_STANDIN_COPY_LAG=str(lag))
    out = subprocess.run([wrap_check, path, str(7 * BLOCK + 1000)], capture_output=True, text=True, timeout=TIMEOUT, env=env)
    assert out.returncode == 0 and clean(out.stderr) and "GPU front end" not in out.stderr, (out.returncode, out.stderr[-2000:])
    assert pdus_of(out.stdout) == list(enumerate(hashes))


def test_push_failure_releases_everything_and_ends(replay, recordings):
    path, _, hashes = recordings["CS16"]
    text = "injected: the fourth push fails"
    out = run(replay, path, "CS16", prefetch=PREFETCH_MAX, copy_lag=3, fail_push=4, fail_text=text)
    assert out.returncode == 0 and clean(out.stderr), (out.returncode, out.stderr[-2000:])
    assert out.stderr.count("GPU front end: " + text + "\n") == 1 and out.stderr.count("GPU front end:") == 1
    assert pdus_of(out.stdout) == list(enumerate(hashes[:3]))


def test_create_failure_ends_without_a_pdu(replay, recordings):
    text = "injected: no device"
    out = run(replay, recordings["CS16"][0], "CS16", fail_create=text)
    assert out.returncode == 0 and clean(out.stderr), (out.returncode, out.stderr[-2000:])
    assert "GPU front end: " + text + "\n" in out.stderr and out.stdout == ""


def feed_live(proc, raw, want_lines):
    """Three blocks, a pause of ten grace periods counted from the moment the program has taken them out of the pipe, two more
    blocks, end of input.  Returns the lines on stdout at the end of the pause (waits for at most `want_lines` of them) and the
    rest of stdout and stderr."""
    grace = min(max(0.25 * BLOCK / LIVE_FS, 0.0005), 0.020)
    blk = BLOCK * BPS["CS16"]
    proc.stdin.write(raw[:3 * blk].tobytes())
    proc.stdin.flush()
    give_up = time.monotonic() + TIMEOUT
    unread = bytearray(4)
    while True:
        fcntl.ioctl(proc.stdin.fileno(), termios.FIONREAD, unread)
        if int.from_bytes(unread, "little") == 0 or time.monotonic() > give_up:
            break
        select.select([], [], [], 0.001)
    pause_ends = time.monotonic() + 10 * grace
    early = b""
    while early.count(b"\n") < want_lines and time.monotonic() < pause_ends:
        if select.select([proc.stdout], [], [], max(0.0, pause_ends - time.monotonic()))[0]:
            early += os.read(proc.stdout.fileno(), 65536)
    select.select([], [], [], max(0.0, pause_ends - time.monotonic()))
    try:
        rest, err = proc.communicate(raw[3 * blk:5 * blk].tobytes(), timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        proc.kill()
        pytest.fail("the program did not end after the end of its input")
    return early.decode(), rest.decode(), err.decode()


def test_live_source_gets_its_pdus_within_the_grace_period(replay, recordings):
    _, raw, hashes = recordings["CS16"]
    proc = run(replay, "-", "CS16", fs=LIVE_FS, stdin=True, prefetch=PREFETCH_MAX, copy_lag=3)
    early, rest, err = feed_live(proc, raw, 3)
    assert proc.returncode == 0 and clean(err), err[-2000:]
    assert pdus_of(early) == list(enumerate(hashes[:3]))              # on stdout before anything more was written
    assert pdus_of(early + rest) == list(enumerate(hashes[:5]))
    proc = run(replay, "-", "CS16", "--bench", fs=LIVE_FS, stdin=True, prefetch=PREFETCH_MAX, copy_lag=3)
    early, rest, err = feed_live(proc, raw, 0)
    assert proc.returncode == 0 and clean(err), err[-2000:]
    rs = json.loads(early + rest)
    assert rs["blocks"] == 5 and rs["pdus"] == 5 and rs["pipeline_drains"] >= 1 and rs["thread_s"]["grace"] > 0


def test_spectrum_file_and_iq_export_together(replay, recordings, tmp_path):
    path, _, hashes = recordings["CS16"]
    # the rate is chosen so that the last whole interval closes on the very last push: its row is not finished when the loop's
    # non-waiting read runs, and only the final wait = 1 pass of the tear-down can write its line
    fs, csv, iq = 20582, tmp_path / "spectrum.csv", tmp_path / "iq"
    iq.mkdir()
    out = run(replay, path, "CS16", "--spectrum-file", str(csv), "--spectrum-interval", "1", "--iq-export-dir", str(iq), fs=fs,
              prefetch=PREFETCH_MAX, copy_lag=3)
    assert out.returncode == 0 and clean(out.stderr), out.stderr[-2000:]
    assert "overwritten" not in out.stderr and "spectrum monitor" not in out.stderr and "iq export" not in out.stderr, out.stderr
    assert pdus_of(out.stdout) == list(enumerate(hashes))
    # interval i ends with the first block k for which k blocks of signal reach i + 1 seconds
    ends = [math.ceil(i * fs / BLOCK) for i in range(1, NBLOCKS * BLOCK // fs + 1)]
    assert len(ends) >= 8 and ends[-1] == NBLOCKS
    lines = csv.read_text().splitlines()
    assert len(lines) == len(ends)
    bins = 256                                                        # 1024 asked for, halved to the stand-in's fft_size / 16
    for row, (line, first, end) in enumerate(zip(lines, [0] + ends, ends)):
        cols = line.split(", ")
        assert len(cols) == 6 + bins and int(cols[5]) == end - first, (row, cols[:6])
        want = [10 * math.log10(float(np.float32((1 + (row * 31 + b) % 97) / 128))) for b in range(bins)]     # the stand-in's row_power()
        assert np.allclose([float(c) for c in cols[6:]], want, atol=0.006), row
    stamps = [line.split(", ")[:2] for line in lines]
    assert stamps == sorted(stamps)
    for s, freq in enumerate((10010000, 10020000)):
        got = np.fromfile(iq / ("%d.cf32" % freq), np.float32).reshape(-1, 2)
        total = sum(1 + (b * 7 + s * 3) % OUT_PER_BLOCK for b in range(NBLOCKS))      # the stand-in's export_count()
        assert len(got) == total
        assert np.array_equal(got[:, 0], np.arange(total, dtype=np.float32)) and np.all(got[:, 1] == s)
