"""CPU tests of what the nine companion bindings share
(hadoofus_amd/companion.py), asked of every module of build.COMPANIONS alike:
importing loads nothing, loading is cached, a missing library and a wrong ABI
version are refused with the library's own name in the message, an error
carries the library's own last-error text, every companion has a module and
every module a companion, and the batch front end the three batch modules share
gives the same answers through each of them.  Everything is host-only."""
import importlib
import os
import pkgutil
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hadoofus_amd import build  # noqa: E402

EINVAL = -1
STEMS = [c[0] for c in build.COMPANIONS]
NOT_BINDINGS = {"abi", "build", "companion", "shard"}  # the package's modules that mirror no companion


@pytest.fixture(scope="module")
def libs():
    """The release library, with every companion beside it, built if stale."""
    return build.build()


def module(stem):
    return importlib.import_module("hadoofus_amd." + stem)


def fresh(code):
    """Run code in an interpreter of its own."""
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_the_table_is_the_nine_companions_in_build_order():
    assert STEMS == ["md5crc", "writev", "wire", "wire_batch", "wirev", "wire_fused", "wire_fused_batch",
                     "wirev_fused", "wirev_fused_batch"]
    for stem, sources, headers, public in build.COMPANIONS:
        up = stem.upper()
        assert build.companion_lib(stem) == getattr(build, up + "_LIB")
        assert build.companion_lib(stem) == os.path.join(build.LIBDIR, f"libhadoofus_{stem}.so")
        assert (sources, headers, public) == (getattr(build, up + "_SOURCES"), getattr(build, up + "_HEADERS"),
                                              getattr(build, up + "_PUBLIC"))
        assert f"{stem}_exports.map" in headers and f"hadoofus_{stem}.h" in public
        assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in sources + headers)


def test_every_companion_has_a_module_and_every_module_a_companion():
    import hadoofus_amd
    names = {m.name for m in pkgutil.iter_modules(hadoofus_amd.__path__)}
    assert names - NOT_BINDINGS == set(STEMS) and len(STEMS) == 9
    for stem in STEMS:
        m = module(stem)
        for name in ("LIB_PATH", "ABI_VERSION", "_lib", "load", "check_abi", "bind", "_check"):
            assert hasattr(m, name), (stem, name)


@pytest.mark.parametrize("stem", STEMS)
def test_import_loads_nothing(stem):
    fresh(f"from hadoofus_amd import abi, companion, {stem} as m\n"
          "assert abi._lib is None and m._lib is None\n")


@pytest.mark.parametrize("stem", STEMS)
def test_loading_is_cached(libs, stem):
    m = module(stem)
    lib = m.load()
    assert lib is not None and m.load() is lib and m._lib is lib
    assert m.LIB_PATH == build.companion_lib(stem) and os.path.dirname(m.LIB_PATH) == os.path.dirname(libs)
    assert getattr(lib, f"hdfs_{stem}_abi_version")() == m.ABI_VERSION


@pytest.mark.parametrize("stem", STEMS)
def test_a_missing_library_is_refused(libs, tmp_path, stem):
    missing = str(tmp_path / f"libhadoofus_{stem}.so")
    fresh(f"from hadoofus_amd import {stem} as m\n"
          f"path = {missing!r}\n"
          "try:\n"
          "    m.load(path=path)\n"
          "except ImportError as e:\n"
          "    assert path in str(e) and 'hadoofus_amd.build' in str(e), e\n"
          "else:\n"
          "    raise SystemExit('a library that is not there was loaded')\n"
          "assert m._lib is None\n"
          "assert m.load() is m._lib is not None\n")  # and the refusal left nothing behind


@pytest.mark.parametrize("stem", STEMS)
def test_a_wrong_abi_is_refused(stem):
    m = module(stem)
    v = m.ABI_VERSION + 1
    other = types.SimpleNamespace(**{f"hdfs_{stem}_abi_version": lambda: v})
    with pytest.raises(ImportError) as e:
        m.check_abi(other)
    assert f"library ABI version {v}, bindings written for {m.ABI_VERSION}" in str(e.value)
    same = types.SimpleNamespace(**{f"hdfs_{stem}_abi_version": lambda: m.ABI_VERSION})
    assert m.check_abi(same) is same


def provoke_einval(stem, m):
    """A host-only call that the library of that stem rejects."""
    if stem == "md5crc":
        return m.file_checksum_from_blocks(bytes(16), ctype=0)  # neither CRC32 nor CRC32C
    if stem == "writev":
        return m.layout([10], offset_in_block=-1)  # its layout takes no proto
    if stem == "wire":
        return m.layout(10, proto=7)
    if stem == "wire_fused":
        return m.packet_records(10, proto=7)  # it has no layout call: the size query
    if stem in ("wirev", "wirev_fused"):
        return m.layout([10], proto=7)
    if stem == "wirev_fused_batch":
        return m.layout([m.write(frags=[(None, 10)])], proto=7)
    return m.layout([m.write(nbytes=10)], proto=7)


@pytest.mark.parametrize("stem", STEMS)
def test_errors_carry_the_librarys_own_text(libs, stem):
    m = module(stem)
    with pytest.raises(m.abi.CRC32CError) as e:
        provoke_einval(stem, m)
    text = getattr(m.load(), f"hdfs_{stem}_last_error")().decode()
    assert text and e.value.code == EINVAL
    assert str(e.value) == f"hadoofus_crc32c error {EINVAL}: {text}"
    with pytest.raises(m.abi.CRC32CError) as e:  # _check itself, with a code of the caller's
        m._check(-5)
    assert e.value.code == -5 and str(e.value) == f"hadoofus_crc32c error -5: {text}"
    assert m._check(0) is None


# ---- the batch front end, through each of the three modules -------------------------------
SIZES = [0, 1, 513, 65537]


def contiguous(m, off, **kw):
    return [m.write(nbytes=n, offset_in_block=off, seqno=100 * k + 3, finish=k == len(SIZES) - 1, **kw)
            for k, n in enumerate(SIZES)]


@pytest.mark.parametrize("off", [0, 4321])
def test_the_shared_batch_front_end_matches(libs, off):
    from hadoofus_amd import companion, wire_batch, wire_fused_batch, wirev_fused_batch
    assert wire_batch.BatchWrite is wire_fused_batch.BatchWrite is companion.BatchWrite
    assert wire_batch.Totals is wire_fused_batch.Totals is companion.Totals
    assert wirev_fused_batch.BatchWrite is not companion.BatchWrite
    # the entries, field by field, with pointers that nothing dereferences
    fields = [f for f, _ in companion.BatchWrite._fields_]
    for query in (False, True):
        a, b = (m.entries(contiguous(m, off, dptr=0x1000, wire_ptr=0x2000, wire_cap=1 << 20), query)
                for m in (wire_batch, wire_fused_batch))
        assert len(a) == len(b) == len(SIZES)
        for k, (x, y) in enumerate(zip(a, b)):
            assert [getattr(x, f) for f in fields] == [getattr(y, f) for f in fields], (query, k)
            assert (x.data, x.len) == (0x1000 if SIZES[k] else None, SIZES[k])
            assert (x.wire, x.wire_cap) == ((None, 0) if query else (0x2000, 1 << 20))
            assert (x.offset_in_block, x.seqno, x.finish) == (off, 100 * k + 3, int(k == len(SIZES) - 1))
    # layout and the size query's records (a size query reads no data)
    outs, tot = wire_batch.layout(contiguous(wire_batch, off))
    assert (outs, tot) == wire_fused_batch.layout(contiguous(wire_fused_batch, off))
    recs = wire_batch.packet_records(contiguous(wire_batch, off))
    assert recs == wire_fused_batch.packet_records(contiguous(wire_fused_batch, off))
    assert [r[0] for r in recs] == [o["wire_len"] for o in outs] and [len(r[1]) for r in recs] == [o["npkts"] for o in outs]
    assert tot["npkts"] == sum(o["npkts"] for o in outs) and recs[-1][1][-1]["last"]
    # the gather batch: the same writes, each as two fragments split at byte 1
    gathered = [wirev_fused_batch.write(frags=[(None, min(1, n)), (None, n - min(1, n))], offset_in_block=off,
                                        seqno=100 * k + 3, finish=k == len(SIZES) - 1) for k, n in enumerate(SIZES)]
    arr, keep = wirev_fused_batch.entries(gathered, True)
    assert len(keep) == len(SIZES) and [e.iovcnt for e in arr] == [2] * len(SIZES)
    gouts, gtot = wirev_fused_batch.layout(gathered)
    assert [dict(o, len=n) for o, n in zip(outs, SIZES)] == gouts
    assert {f: gtot[f] for f in tot} == tot
    assert wirev_fused_batch.packet_records(gathered) == recs
