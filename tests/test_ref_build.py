"""oracle/ref_build.py: the recipe that compiles the reference's WSHandler.cpp.
Where the reference checkout is absent it does nothing and touches nothing;
where it is present it leaves both libraries, and what they export is the
wrapper's ABI.  No GPU needed."""
import ctypes as C
import os

import pytest

from oracle import ref_build

HAVE_REF = os.path.exists(ref_build.reference_source())


def test_absent_reference_builds_nothing_and_touches_nothing(tmp_path):
    out = tmp_path / "_ref"
    out.mkdir()
    keep = out / "libkmws_ref_O3.so"
    keep.write_bytes(b"built elsewhere")
    before = os.stat(keep).st_mtime_ns
    assert ref_build.build(reference=str(tmp_path / "no_checkout_here"), out_dir=str(out)) == {}
    assert sorted(p.name for p in out.iterdir()) == ["libkmws_ref_O3.so"]
    assert keep.read_bytes() == b"built elsewhere" and os.stat(keep).st_mtime_ns == before
    # and a directory that does not exist is not created
    assert ref_build.build(reference=str(tmp_path / "no_checkout_here"), out_dir=str(tmp_path / "none")) == {}
    assert not (tmp_path / "none").exists()


@pytest.mark.skipif(not HAVE_REF, reason="reference checkout not present")
def test_recipe_builds_both_libraries(tmp_path):
    built = ref_build.build(out_dir=str(tmp_path))
    assert sorted(built) == ["O0", "O3"]
    for opt, path in built.items():
        assert path == ref_build.lib_path(opt, str(tmp_path)) and os.path.getsize(path) > 0
        L = C.CDLL(path)
        for sym in ("ref_mask", "ref_mask_chain", "ref_encode_header", "ref_decoder_create", "ref_decoder_destroy",
                    "ref_decoder_reset", "ref_decoder_set_mode", "ref_decoder_feed"):
            assert hasattr(L, sym), (opt, sym)
        assert not hasattr(L, "ref_decoder_state")
    # the header copy: the one token, nothing else
    src = open(os.path.join(ref_build.REFERENCE, "include", "kmbuffer.h")).read()
    got = (tmp_path / "include" / "kmbuffer.h").read_text()
    assert got == src.replace("auto* createSharedData(", "_SharedBase* createSharedData(") and got != src
    assert not [p for p in os.listdir(tmp_path) if p.endswith(".tmp")]


def test_ref_dir_is_ignored_by_git():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "oracle/_ref/" in open(os.path.join(root, ".gitignore")).read().split()
