"""Pins the CPU oracle (oracle/kmws_oracle.c) to the RFC 6455 known answers and
the transcribed values of tests/golden/reference_vectors.json, and to
tests/golden/reference_recorded.json: the outputs of kuma's own compiled
WSHandler.cpp, recorded by make_reference_vectors.py --record.  The recorded
file needs no reference to be checked, so it runs everywhere; where the
reference is built it is recorded again in memory, so a stale file fails.
No GPU needed."""
import hashlib
import importlib.util
import json
import os

import pytest

import ref_cases as rc
from oracle import oracle as orc

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.json")))
RECORDED_PATH = os.path.join(os.path.dirname(__file__), "golden", "reference_recorded.json")
RECORDED = json.load(open(RECORDED_PATH))
MODES = {"CLIENT": orc.CLIENT, "SERVER": orc.SERVER}


def gen(name, n):
    if name == "zeros":
        return bytes(n)
    if name == "iota":
        return bytes(i & 0xFF for i in range(n))
    raise ValueError(name)


def case_input(c):
    data = bytes.fromhex(c["input_hex"])
    if "tail_gen" in c:
        data += gen(c["tail_gen"], c["tail_len"])
    return data


def expected_payload(f):
    if "payload_hex" in f:
        return bytes.fromhex(f["payload_hex"])
    return gen(f["payload_gen"], f["length"])


@pytest.mark.parametrize("c", GOLD["decode"], ids=lambda c: c["name"])
def test_decode_golden(c):
    d = orc.Decoder(MODES[c["mode"]])
    data = case_input(c)
    rets = []
    if c["chunk"] <= 0:
        rets.append(d.feed(data))
    else:
        for i in range(0, len(data), c["chunk"]):
            rets.append(d.feed(data[i:i + c["chunk"]]))
    assert rets == c["expect_rets"]
    assert len(d.frames) == len(c["expect_frames"])
    for got, exp in zip(d.frames, c["expect_frames"]):
        for k in ("fin", "rsv1", "rsv2", "rsv3", "opcode", "mask", "length"):
            assert getattr(got, k) == exp[k], k
        assert got.maskey.hex() == exp["maskey"]
        assert got.payload == expected_payload(exp)
    for step in c.get("then", []):
        assert d.feed(bytes.fromhex(step["input_hex"])) == step["expect_rets"][0]


@pytest.mark.parametrize("c", GOLD["encode"], ids=lambda c: c["name"])
def test_encode_golden(c):
    h = orc.Hdr(fin=c["fin"], rsv1=c["rsv1"], rsv2=c["rsv2"], rsv3=c["rsv3"], opcode=c["opcode"],
                mask=c["mask"], maskey=bytes.fromhex(c["maskey"]), length=c["length"])
    assert orc.encode_header(h).hex() == c["expect_hex"]


@pytest.mark.parametrize("c", GOLD["mask"], ids=lambda c: c["name"])
def test_mask_golden(c):
    key = bytes.fromhex(c["key"])
    segs = [bytes.fromhex(s) for s in c["segments_hex"]]
    assert [s.hex() for s in orc.mask_chain(key, segs)] == c["expect_hex"]


@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 13, 4096])
def test_chunking_invariance(chunk):
    """any chunking yields identical callbacks."""
    import random
    rng = random.Random(1234 + chunk)
    stream = b""
    for i in range(40):
        n = rng.choice([0, 1, 5, 125, 126, 127, 300, 65535, 65536, 70000])
        key = bytes(rng.randrange(256) for _ in range(4))
        payload = bytes(rng.randrange(256) for _ in range(n))
        h = orc.Hdr(fin=rng.randrange(2), opcode=rng.choice([0, 1, 2]), mask=1, maskey=key, length=n)
        stream += orc.encode_header(h) + orc.mask_bytes(key, payload)
    _, whole = orc.decode_chunks(stream, orc.SERVER, 0)
    rets, parts = orc.decode_chunks(stream, orc.SERVER, chunk)
    assert [f.key() for f in parts] == [f.key() for f in whole]
    assert len(whole) == 40
    assert rets[-1] == 0 and all(r in (0, 1) for r in rets)


# ------------------------------ the recorded fixture ------------------------------
def test_recorded_file_is_what_it_says():
    assert RECORDED["recorded_from"] == "libkmws_ref_O3"
    assert os.path.getsize(RECORDED_PATH) < 200 * 1000
    names = {c["name"] for c in RECORDED["decode"]}
    assert {c["name"] for c in GOLD["decode"]} <= names
    assert {c["name"] for c in rc.streaming_cases()} <= names
    assert len(RECORDED["encode"]) == len(GOLD["encode"]) + len(rc.encode_table_fixture())
    assert len(RECORDED["mask"]) == len(GOLD["mask"]) + len(rc.mask_table_fixture())


@pytest.mark.parametrize("c", RECORDED["decode"], ids=lambda c: c["name"])
def test_decode_recorded(c):
    """Return codes of every feed, every frame field the file holds (all eleven:
    payloads above 256 bytes by SHA-256) and the `then` steps."""
    rc.check_decode(orc, c)


def test_encode_recorded():
    for c in RECORDED["encode"]:
        assert rc.encode_run(orc, c) == c["expect_hex"], c["name"]


def test_mask_recorded():
    for c in RECORDED["mask"]:
        assert rc.mask_run(orc, c) == c["expect_hex"], c["name"]


def test_transcribed_values_equal_recorded_ones():
    """Where a case stands in both files the recording is the authority."""
    for sect, keys in (("decode", ("expect_rets",)), ("encode", ("expect_hex",)), ("mask", ("expect_hex",))):
        rec = {c["name"]: c for c in RECORDED[sect]}
        for c in GOLD[sect]:
            r = rec[c["name"]]
            for k in keys:
                assert r[k] == c[k], (sect, c["name"], k)
            for a, b in zip(c.get("expect_frames", []), r.get("expect_frames", [])):
                for k, v in a.items():
                    if k not in ("payload_hex", "payload_gen"):
                        assert b[k] == v, (c["name"], k)
                want = expected_payload(a)
                if "payload_hex" in b:
                    assert bytes.fromhex(b["payload_hex"]) == want, c["name"]
                else:
                    assert b["payload_sha256"] == hashlib.sha256(want).hexdigest(), c["name"]
            assert len(c.get("expect_frames", [])) == len(r.get("expect_frames", []))
            for a, b in zip(c.get("then", []), r.get("then", [])):
                assert a["expect_rets"] == b["expect_rets"], c["name"]


@pytest.mark.skipif(orc.reference("O3") is None,
                    reason="oracle/_ref/libkmws_ref_O3.so not built (the reference checkout was absent "
                           "when build() ran)")
def test_recorded_file_is_current():
    """Recording again from the built reference gives the committed file, byte for byte."""
    spec = importlib.util.spec_from_file_location(
        "make_reference_vectors", os.path.join(os.path.dirname(__file__), "golden", "make_reference_vectors.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.dumps_recorded(m.recorded(orc.reference("O3"))) == open(RECORDED_PATH).read()
