"""GPU: the sharded HIP path of bench.py (BASELINE configs[4], SURVEY 8 e).

`bench.py --gpus 2 --dist-backend gloo` starts its two rank processes itself
(one GPU per rank; on a one-GPU box both share it), each rank generates its
own shard of a fixed job on the device, unmasks it with the product kernels
in resident sub-batches, and verifies every byte with the device checker.
The test reads rank 0's JSON line: two ranks, contiguous shards covering the
job, sub-batches covering each shard, no mismatches, a clean status word."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, timeout=300, full=True):
    """bench.py's one JSON line; --full unless told otherwise: these tests read
    the legs beside the headline (verify, cfg5_job, plain rate)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *(["--full"] if full else []), *args],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]  # ONE JSON line, whatever the ranks' libraries print
    return json.loads(lines[0])


@pytest.mark.parametrize("job,max_batch", [(65536, 16384), (50001, 20000)])
def test_bench_two_ranks_shard_the_job(job, max_batch):
    d = run_bench("--gpus", "2", "--dist-backend", "gloo", "--job-frames", str(job), "--max-batch-frames",
                  str(max_batch), "--steps", "3", "--warmup", "1", "--cpu-seconds", "0", "--e2e-gib", "0")
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["verify"]["byte_mismatches"] == 0 and d["verify"]["status_word"] == 0
    ranks = sorted(d["ranks"], key=lambda r: r["rank"])
    assert [r["rank"] for r in ranks] == [0, 1]
    assert ranks[0]["frames"][0] == 0 and ranks[-1]["frames"][1] == job
    assert ranks[0]["frames"][1] == ranks[1]["frames"][0]
    for r in ranks:
        subs = r["sub_batches"]
        assert subs[0][0] == r["frames"][0] and subs[-1][1] == r["frames"][1]
        assert all(a[1] == b[0] for a, b in zip(subs, subs[1:]))
        assert all(hi - lo <= max_batch for lo, hi in subs)
        assert r["byte_mismatches"] == 0
    assert len({len(r["sub_batches"]) for r in ranks}) == 1  # the barriers pair up
    assert d["value"] > 0 and d["config"]["total_frames"] == job


def test_bench_one_gpu_small_batch_plain_rate():
    """N = 1 weak scaling on a small batch, default placement: the timed batch
    is a plain allocation, so the plain rate is the headline's own."""
    d = run_bench("--frames", "16384", "--steps", "3", "--warmup", "1", "--cpu-seconds", "0", "--cfg5-anchor", "0",
                  "--e2e-gib", "0")
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["verify"]["byte_mismatches"] == 0
    assert d["config"]["placement"]["kind"] == "plain torch.empty"
    assert d["roofline"]["frac_plain"] == d["roofline"]["frac"] > 0  # the timed batch is the plain allocation


def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times the headline and nothing else -- the side
    legs' keys are null -- and --dump-outputs writes what the last timed step
    left in the batch: here 96 x 64 KiB frames (6 MiB, above bench.DUMP_SAMPLE,
    so the sampled path) after 2 + 3 passes, an odd count, so the unmasked
    payload.  Every array equals the oracle's unmask of the same synthetic
    input, regenerated here from the seeds bench.py documents."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from kuma_amd import kmws
    from oracle import oracle as orc
    n, L, steps, warmup = 96, 65536, 3, 2
    out = tmp_path / "dump"
    d = run_bench("--gpus", "1", "--frames", str(n), "--steps", str(steps), "--warmup", str(warmup),
                  "--dump-outputs", str(out), full=False)
    assert d["full"] is False and d["steps"] == steps and d["warmup"] == warmup
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["config"]["total_frames"] == n
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "GiB/s" and d["dtype"] == "u8"
    assert d["metric"] == bench.METRIC and d["higher_is_better"] is True
    assert d["cfg5_job"] is None and d["e2e_host"] is None and d["cpu_baseline"] is None
    assert d["plain_allocation"] is None and d["verify"] == {"status_word": 0, "byte_mismatches": None}

    seed = 0x6B756D61  # bench.py --seed default
    span = n * L
    base = torch.empty(span, dtype=torch.uint8, device="cuda")
    descs = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    kmws.fill_uniform_descs(descs, L, L, seed ^ 0x5EED)
    kmws.fill_synthetic(base, seed)
    torch.cuda.synchronize()
    want = base.cpu().numpy()
    hd = descs.cpu().numpy().reshape(-1).view(orc.DESC_DTYPE)
    assert hd.shape == (n,) and int(hd["off"][5]) == 5 * L and int(hd["len"][5]) == L
    for _ in range((steps + warmup) % 2):
        orc.unmask_batch(want, hd)

    got = {p.name[:-4]: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["frame_byte_sums", "payload_head", "payload_sample", "payload_tail", "status"]
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 * 10**6
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    pos = np.sort(np.random.default_rng(seed).integers(0, span, size=bench.DUMP_SAMPLE, dtype=np.int64))
    assert np.array_equal(got["payload_sample"], want[pos].astype(np.float32))
    assert np.array_equal(got["payload_head"], want[:L].astype(np.float32))
    assert np.array_equal(got["payload_tail"], want[-L:].astype(np.float32))
    assert np.array_equal(got["frame_byte_sums"], want.reshape(n, L).sum(axis=1, dtype=np.int64).astype(np.float64))
    assert np.array_equal(got["status"], np.zeros(1))


CFG5_FRAMES = 10485760  # BASELINE configs[4]: 10 M x 64 KiB = 640 GiB
CFG5_BATCH = 1310720    # bench.py --max-batch-frames default: 80 GiB resident per sub-batch
_cfg5 = {}


def _check_cfg5(d, world):
    assert d["n_gpus"] == world and d["scaling"] == "strong"
    assert d["config"]["total_frames"] == CFG5_FRAMES and d["config"]["frame_len"] == 65536
    _check_cfg5_ranks(d, world)


def _check_cfg5_ranks(d, world):
    assert d["verify"]["byte_mismatches"] == 0 and d["verify"]["status_word"] == 0
    ranks = sorted(d["ranks"], key=lambda r: r["rank"])
    assert [r["rank"] for r in ranks] == list(range(world))
    assert ranks[0]["frames"][0] == 0 and ranks[-1]["frames"][1] == CFG5_FRAMES
    assert all(a["frames"][1] == b["frames"][0] for a, b in zip(ranks, ranks[1:]))  # contiguous shards
    for r in ranks:
        subs = r["sub_batches"]
        assert len(subs) == 8 // world
        assert subs[0][0] == r["frames"][0] and subs[-1][1] == r["frames"][1]
        assert all(a[1] == b[0] for a, b in zip(subs, subs[1:]))
        assert all(hi - lo == CFG5_BATCH for lo, hi in subs)
        assert r["byte_mismatches"] == 0
    assert d["value"] > 0


@pytest.mark.timeout(600)
def test_cfg5_job_anchor_at_one_gpu():
    """the N = 1 line (cfg2, here on a small batch) also carries
    `cfg5_job`, BASELINE configs[4]'s real job -- 10,485,760 x 64 KiB frames as 8
    resident sub-batches of 1,310,720 frames (80 GiB), each generated on the
    device, timed as the N > 1 lines time their ranks' sub-batches, verified
    byte for byte: the same-job anchor of the 1 -> 8 curve."""
    d = run_bench("--gpus", "1", "--frames", "16384", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0",
                  "--e2e-gib", "0", timeout=600)
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["config"]["total_frames"] == 16384
    c = d["cfg5_job"]
    assert c["total_frames"] == CFG5_FRAMES and c["sub_batches"] == 8 and c["resident_batch_frames"] == CFG5_BATCH
    assert c["scaling"] == "strong" and c["frame_len"] == 65536
    _check_cfg5_ranks(c, 1)
    assert d["verify"]["byte_mismatches"] == 0
    _cfg5[1] = c["value"]


@pytest.mark.timeout(600)
def test_cfg5_full_job_two_ranks_share_the_gpu():
    """The same job at --gpus 2 (gloo harness, both ranks on the one GPU of the
    box): 4 sub-batches per rank over contiguous shards, every byte verified;
    the two ranks share one GPU's HBM, so the aggregate must stay within 10 %
    of the N = 1 line's cfg5_job value, the same job timed the same way
    (nothing is lost to the partition or the harness)."""
    d = run_bench("--gpus", "2", "--dist-backend", "gloo", "--job-frames", str(CFG5_FRAMES), "--steps", "2",
                  "--warmup", "1", "--cpu-seconds", "0", "--e2e-gib", "0", timeout=600)
    _check_cfg5(d, 2)
    assert d["cfg5_job"] is None  # the N > 1 headline is the job itself
    if 1 in _cfg5:
        assert abs(d["value"] / _cfg5[1] - 1) <= 0.10, (d["value"], _cfg5[1])
