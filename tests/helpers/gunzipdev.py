"""TEST INFRASTRUCTURE: the bodies of the device gunzip tests (test_gpu_gunzip.py runs them on the GPU, test_emu_gunzip.py on the kernel emulator).

Every yardstick is Python's zlib / gzip, never the code under test: a device output is accepted when it equals what zlib inflates the same
bytes to, and a refusal when zlib refuses the same bytes.  helpers/inflatepy.py, a plain-Python inflate that is itself checked against zlib
on every blob it is used for, says where blocks and members begin, i.e. where the decoder's tasks must start; its DEFLATE writer makes the
streams zlib never emits (a distance of 32 768, a reference in front of a member's first byte).  smr_gunzip_info must say "device" wherever a
test is about the kernels: the host path inside the same call would otherwise hide a broken kernel."""
import ctypes as C
import gzip
import os
import random
import zlib

import numpy as np
import pytest

import sortmerna_amd as smr
from sortmerna_amd import engine as smr_engine

from . import inflatepy as ip
from .gzipdev import AMPLICON, members, seeded, texty

ERR_ARG, ERR_IO, ERR_CAPACITY = -1, -2, -4
GRAINS = (1, 0)


# ------------------------------------------------------------------------------------------------ inputs
def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, wbits=31):
    z = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if not flush_every:
        return z.compress(data) + z.flush()
    out = b""
    for at in range(0, len(data), flush_every):
        out += z.compress(data[at:at + flush_every]) + z.flush(zlib.Z_SYNC_FLUSH)
    return out + z.flush()


def fastq(n_reads, seed):
    rng = random.Random(seed)
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(rng.choice(b"ACGT") for _ in range(150)), bytes(33 + rng.randrange(40) for _ in range(150))) for i in range(n_reads))


_round_trip = {}
ROUND_TRIP = ["the empty member", "1 byte", "level 1", "level 6", "level 9", "level 0, several stored blocks", "Z_FIXED", "Z_HUFFMAN_ONLY", "Z_RLE",
              "a sync flush every 20 000 bytes", "seeded FASTQ, level 6"]


def round_trip_inputs():
    """name -> gzip bytes"""
    if not _round_trip:
        t = texty(120_000, 7) + fastq(1000, 6)            # (lines that repeat, then reads that do not: a few long blocks, then many)
        _round_trip.update({
            "the empty member": deflate(b""), "1 byte": deflate(b"G"), "level 1": deflate(t, 1), "level 6": deflate(t, 6), "level 9": deflate(t, 9),
            "level 0, several stored blocks": deflate(texty(200_000, 8), 0), "Z_FIXED": deflate(t, 6, zlib.Z_FIXED), "Z_HUFFMAN_ONLY": deflate(t, 6, zlib.Z_HUFFMAN_ONLY),
            "Z_RLE": deflate(t, 6, zlib.Z_RLE), "a sync flush every 20 000 bytes": deflate(t, 6, flush_every=20_000), "seeded FASTQ, level 6": deflate(fastq(1200, 5), 6)})
        assert list(_round_trip) == ROUND_TRIP
    return _round_trip


def on_device(e, blob, grain, what):
    """blob through the device decoder: zlib's bytes, and the device path"""
    got = e.gunzip_batch(blob, grain)
    info = e.gunzip_info()
    print("%s, grain %d: %s" % (what, grain, info))
    assert info["path"] == "device", "%s, grain %d: the host inflated (%s)" % (what, grain, info["why"])
    assert got == gzip.decompress(blob), "%s, grain %d: not zlib's bytes" % (what, grain)
    assert info["compressed"] == len(blob) and info["plain"] == len(got), what
    return info


def starts_equal_the_models(e, blob, what):
    """after a call with grain = 1: the tasks the search found are the model's starts; a task the stitch made costs a round and is said so"""
    tasks, info = e.gunzip_tasks(), e.gunzip_info()
    found = [(bit, hdr) for bit, hdr, extra in tasks if not extra]
    assert found == ip.task_starts(blob), "%s: task starts %s, the model's %s" % (what, found[:8], ip.task_starts(blob)[:8])
    extra = [t for t in tasks if t[2]]
    assert info["rounds"] == 1 + len(extra) and info["tasks"] == len(tasks), (what, info)
    if extra:
        print("%s: %d tasks made by the stitch (a false or missing candidate): %s" % (what, len(extra), extra))
    return info


def round_trip_body(name):
    blob = round_trip_inputs()[name]
    e = smr.Engine(0)
    try:
        for grain in GRAINS:
            info = on_device(e, blob, grain, name)
            if grain == 1:
                starts_equal_the_models(e, blob, name)
                _, blocks, mem = ip.model(blob)
                assert info["members"] == len(mem) == 1
                assert (info["stored"], info["fixed"], info["dynamic"]) == tuple(sum(1 for b in blocks if b[1] == k) for k in range(3)), (name, info)
        if name == "level 0, several stored blocks":
            assert info["stored"] >= 4 and info["dynamic"] == 0
        if name in ("level 6", "a sync flush every 20 000 bytes", "seeded FASTQ, level 6"):
            assert len(ip.task_starts(blob)) >= 10, "the input has too few blocks to test anything"
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ placeholders
def far_repeat_blob():
    """40 000 bytes from zlib up to a sync flush, then a dynamic block that begins with 258 bytes from distance exactly 32 768: byte 0 of the
    window in front of the task that starts there"""
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    w = ip.Writer()
    w.raw(z.compress(texty(40_000, 21)) + z.flush(zlib.Z_SYNC_FLUSH))
    w.dynamic([(258, 32768), ord("x"), (100, 32768), (30, 1), (258, 32767)])
    w.end_fixed()
    raw = w.bytes()
    return ip.member(raw, ip.raw_inflate(raw))


def six_copies_blob(crafted):
    """one block of 32 KiB of lines six times over.  crafted: copies 2 .. 6 are dynamic blocks of nothing but matches at distance 32 768 (zlib
    itself reaches back 32 506 bytes at the most), so every task but the first is placeholders only and is resolved through all its
    predecessors; else zlib's own stream with a sync flush behind every copy"""
    block = texty(32768, 22)
    if not crafted:
        return deflate(block * 6, 6, flush_every=32768)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    w = ip.Writer()
    w.raw(z.compress(block) + z.flush(zlib.Z_SYNC_FLUSH))
    for _ in range(5):
        w.dynamic([(258, 32768)] * 126 + [(130, 32768)] * 2)
    w.end_fixed()
    raw = w.bytes()
    assert ip.raw_inflate(raw) == block * 6
    return ip.member(raw, block * 6)


def short_task_blob():
    """a task of 5 000 bytes between two of 100 000: its window keeps 27 768 bytes of the one in front of it"""
    t = texty(205_000, 23)
    z = zlib.compressobj(6, zlib.DEFLATED, 31)
    return z.compress(t[:100_000]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(t[100_000:105_000]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(t[105_000:]) + z.flush()


def placeholders_body():
    e = smr.Engine(0)
    try:
        far = far_repeat_blob()
        on_device(e, far, 1, "a repeat at distance 32 768")
        starts_equal_the_models(e, far, "a repeat at distance 32 768")
        assert len(e.gunzip_tasks()) >= 3
        on_device(e, far, 0, "a repeat at distance 32 768")
        for crafted in (True, False):
            blob = six_copies_blob(crafted)
            on_device(e, blob, 1, "six copies of 32 KiB (%s)" % ("matches only" if crafted else "zlib's"))
            starts_equal_the_models(e, blob, "six copies")
            if crafted:
                assert [t[0] for t in e.gunzip_tasks()][-5:] == [b[0] for b in ip.model(blob)[1] if b[1] == 2 and not b[2]][-5:] and len(e.gunzip_tasks()) >= 6
            on_device(e, blob, 0, "six copies of 32 KiB")
        short = short_task_blob()
        on_device(e, short, 1, "a short task between two long ones")
        starts_equal_the_models(e, short, "a short task between two long ones")
        on_device(e, short, 0, "a short task between two long ones")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ members
def header(flags, name=b"reads.fq", extra=b"\x41\x42\x03\x00xyz", comment=b"made by a test"):
    h = b"\x1f\x8b\x08" + bytes([flags]) + b"\x15\xcd\x5b\x07\x02\x03"
    if flags & 4:
        h += len(extra).to_bytes(2, "little") + extra
    if flags & 8:
        h += name + b"\0"
    if flags & 16:
        h += comment + b"\0"
    if flags & 2:
        h += (zlib.crc32(h) & 0xFFFF).to_bytes(2, "little")
    return h


def five_members():
    parts = [texty(70_000, 31), b"", texty(3, 32), fastq(300, 33), texty(40_000, 34)]
    flags = [8, 4, 16, 2, 2 | 4 | 8 | 16]
    return b"".join(ip.member(deflate(p, 6, wbits=-15), p, header(f)) for p, f in zip(parts, flags)), parts


def members_body():
    e = smr.Engine(0)
    try:
        blob, parts = five_members()
        assert members(blob) == parts                         # (zlib takes the headers, FHCRC included)
        for grain in GRAINS:
            info = on_device(e, blob, grain, "five members")
            assert info["members"] == 5
        on_device(e, blob, 1, "five members")
        starts_equal_the_models(e, blob, "five members")
        assert sum(1 for t in e.gunzip_tasks() if t[1]) == 5
        # a header CRC that is wrong: zlib refuses, and so does the call
        bad = bytearray(blob)
        at = ip.model(blob)[2][3][1]                           # first data byte of member 3: its FHCRC lies in front of it
        bad[at - 1] ^= 1
        refusal_equals_zlibs(e, bytes(bad), "a wrong header CRC")
        # what the device compressor writes: 2 C + 1 bytes are three members, each a task
        c = e.gzip_chunk()
        data = texty(2 * c + 1, 35)
        gz = e.gzip_batch([data])[0]
        for grain in GRAINS:
            got = e.gunzip_batch(gz, grain)
            assert e.gunzip_info()["path"] == "device" and got == data
        assert e.gunzip_batch(gz, 1) == data and e.gunzip_tasks() == [(8 * m[0], True, False) for m in ip.model(gz)[2]] and len(e.gunzip_tasks()) == 3
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ a false candidate
def false_candidate_blob(fixed_behind):
    """the bytes of a byte-aligned non-final dynamic block -- what zlib writes behind a sync flush, up to the next one -- as the payload of a
    stored block; behind it zlib's stream (fixed_behind: fixed-Huffman blocks, which are no candidates, so that the stored block's end hits no
    task start and the stitch makes a task there)"""
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    z.compress(texty(30_000, 41))
    z.flush(zlib.Z_SYNC_FLUSH)
    chunk = z.compress(fastq(150, 42)) + z.flush(zlib.Z_SYNC_FLUSH)
    assert len(chunk) <= 65535 and chunk[0] & 7 == 4         # BFINAL 0, BTYPE 2 at bit 0
    w = ip.Writer()
    w.stored(chunk)
    z2 = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED if fixed_behind else zlib.Z_DEFAULT_STRATEGY)
    w.raw(z2.compress(fastq(500, 43)) + z2.flush())
    raw = w.bytes()
    return ip.member(raw, ip.raw_inflate(raw)), (10 + 5) * 8


def false_candidate_body():
    e = smr.Engine(0)
    try:
        for fixed_behind in (False, True):
            blob, false_bit = false_candidate_blob(fixed_behind)
            info = on_device(e, blob, 1, "a false candidate")
            tasks = e.gunzip_tasks()
            assert false_bit not in [t[0] for t in tasks], "the false candidate is a confirmed task"
            assert info["candidates"] > len([t for t in tasks if not t[2]]), "the search did not find the embedded block header"
            starts_equal_the_models(e, blob, "a false candidate")
            assert info["rounds"] == (2 if fixed_behind else 1), info
            on_device(e, blob, 0, "a false candidate")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ refusals
def zlib_refuses(blob):
    """what zlib says to blob: None (it inflates), "truncated" or "corrupt" -- the verdicts of the library's host inflate"""
    rest = blob
    try:
        while rest:
            d = zlib.decompressobj(31)
            d.decompress(rest)
            if not d.eof:
                return "truncated"
            rest = d.unused_data
    except zlib.error:
        return "corrupt"
    return None


def refusal_equals_zlibs(e, blob, what):
    verdict = zlib_refuses(blob)
    assert verdict, "%s: zlib takes it" % what
    L = e.L
    gz = np.frombuffer(blob, dtype=np.uint8)
    need = C.c_uint64(7)
    buf = np.full(1 << 20, 0xA5, dtype=np.uint8)
    for plain, cap in ((None, 0), (buf.ctypes.data, buf.size)):
        rc = L.smr_gunzip_batch(e.h, gz.ctypes.data, len(blob), 1, plain, cap, C.byref(need))
        msg = L.smr_last_error(e.h).decode()
        assert rc == ERR_IO and msg == "smr_gunzip_batch: %s gzip stream" % verdict, "%s: %d, %r; zlib says %s" % (what, rc, msg, verdict)
        assert need.value == 0 and (buf == 0xA5).all() and e.gunzip_info()["path"] == "host", what
    print("%s: %s" % (what, e.gunzip_info()))


def refusal_blobs():
    t = texty(150_000, 51)
    good = deflate(t, 6)
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x10
    wrong_crc = bytearray(good)
    wrong_crc[-8] ^= 1
    wrong_isize = bytearray(good)
    wrong_isize[-4] ^= 1
    w = ip.Writer()
    w.bits(1, 1)
    w.bits(3, 2)
    btype3 = ip.member(w.bytes() + b"\0" * 8, b"")
    w = ip.Writer()
    w.dynamic([ord("A"), (3, 2)], final=True)
    too_far = ip.member(w.bytes(), b"AAAA")
    two = deflate(t[:50_000], 6) + bytes(too_far)
    return good, {"a flipped payload bit": bytes(flipped), "a wrong CRC": bytes(wrong_crc), "a wrong ISIZE": bytes(wrong_isize), "a file cut in the middle": good[:len(good) // 2],
                  "a file cut inside its trailer": good[:-3], "bytes behind the last member": good + b"reads", "BTYPE 3": btype3,
                  "a too-far distance at a member start": too_far, "a too-far distance at the start of a second member": two}


def refusals_body():
    e = smr.Engine(0)
    try:
        good, bad = refusal_blobs()
        for what, blob in bad.items():
            refusal_equals_zlibs(e, blob, what)
            on_device(e, good, 1, "a good file after " + what)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ the contract of smr_gunzip_batch
def contract_body():
    e, e2 = smr.Engine(0), smr.Engine(0)
    L = e.L
    try:
        blob = round_trip_inputs()["seeded FASTQ, level 6"]
        want = gzip.decompress(blob)
        gz = np.frombuffer(blob, dtype=np.uint8)
        need = C.c_uint64(7)
        assert L.smr_gunzip_batch(e.h, gz.ctypes.data, len(blob), 0, None, 0, C.byref(need)) == 0 and need.value == len(want)
        buf = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
        need.value = 7
        assert L.smr_gunzip_batch(e.h, gz.ctypes.data, len(blob), 0, buf.ctypes.data, len(want) - 1, C.byref(need)) == ERR_CAPACITY
        assert need.value == len(want) and (buf == 0xA5).all() and b"smr_gunzip_batch" in L.smr_last_error(e.h)
        assert L.smr_gunzip_batch(e.h, gz.ctypes.data, len(blob), 0, buf.ctypes.data, len(want) + 64, C.byref(need)) == 0
        assert need.value == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()
        assert e.gunzip_info()["path"] == "device"
        # the same bytes: twice, under either grain, on another context
        assert e.gunzip_batch(blob) == want and e.gunzip_batch(blob, 1) == want and e2.gunzip_batch(blob) == want
        t1 = e.gunzip_tasks()
        assert e.gunzip_batch(blob, 1) == want and e.gunzip_tasks() == t1
        # NULL arguments
        assert L.smr_gunzip_batch(None, gz.ctypes.data, len(blob), 0, None, 0, C.byref(need)) == ERR_ARG
        assert L.smr_gunzip_batch(e.h, None, len(blob), 0, None, 0, C.byref(need)) == ERR_ARG
        assert L.smr_gunzip_batch(e.h, gz.ctypes.data, len(blob), 0, None, 0, None) == ERR_ARG
        assert L.smr_gunzip_info(e.h, None) == ERR_ARG and L.smr_gunzip_times(e.h, None) == ERR_ARG and L.smr_gunzip_tasks(e.h, None, 0, None) == ERR_ARG
        assert e.gunzip_batch(blob) == want
        ms = e.gunzip_times()
        assert list(ms) == ["h2d", "find", "count", "write", "window", "resolve"] and all(v >= 0 for v in ms.values()) and ms["count"] > 0
        # bytes that are no gzip file, and no bytes: the host's refusal
        for junk in (b"", b"\x1f", b"@r1\nACGT\n+\nIIII\n" * 4):
            with pytest.raises(smr.SmrError):
                e.gunzip_batch(junk)
            assert e.gunzip_info()["path"] == "host" and zlib_refuses(junk or b"\0")
        assert e.gunzip_batch(blob) == want
    finally:
        e.close()
        e2.close()


def sparse_body():
    """17 MiB of text in stored blocks have one candidate, the member header: more than 16 MiB per candidate is serial work for one wave, and the
    call says so and lets zlib inflate"""
    data = (texty(100_000, 61) * 180)[:17 << 20]
    blob = deflate(data, 0)
    e = smr.Engine(0)
    try:
        assert e.gunzip_batch(blob) == data
        info = e.gunzip_info()
        assert info["path"] == "host" and info["why"] == "not taken" and info["candidates"] == 1, info
        on_device(e, round_trip_inputs()["level 0, several stored blocks"], 0, "a small file of stored blocks")
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ smr_reads_upload_fastx* under SMR_FASTX_INFLATE
def upload_body(is_fastq, n_rec, tmp_path):
    from test_gpu_fastx_device import same_reads, scan_text
    data = scan_text(is_fastq, n_rec)
    path = os.path.join(str(tmp_path), "reads.%s.gz" % ("fq" if is_fastq else "fa"))
    blob = deflate(data, 6)
    with open(path, "wb") as f:
        f.write(blob)
    e = smr.Engine(0)
    try:
        want = e.upload_fastx(path, 2, keep=True)
        info_want, split_want = e.fastx_info(), e.fastx_split(hit=[i % 3 == 0 for i in range(n_rec)])
        try:
            for src in (path, blob):
                for view in (False, True):
                    got = e.upload_fastx(src, 2, view=view, keep=True, inflate=True)
                    try:
                        what = "%d records, %s, view %s" % (n_rec, "the file" if src is path else "bytes", view)
                        assert e.gunzip_info()["path"] == "device" and e.gunzip_info()["plain"] == len(data), what
                        assert e.fastx_info() == info_want and info_want[0] == 0, (what, e.fastx_info(), info_want)
                        same_reads(got, want, what, view)
                        assert e.fastx_split(hit=[i % 3 == 0 for i in range(n_rec)]) == split_want, what
                    finally:
                        got.free()
            # without a Reads object only the totals cross the bus; the batch is the same
            assert e.L.smr_reads_upload_fastx_file(e.h, path.encode(), 2, smr_engine.FASTX_KEEP | smr_engine.FASTX_INFLATE, None, None, 0) == 0
            assert e.fastx_info() == info_want and e.fastx_split(hit=[i % 3 == 0 for i in range(n_rec)]) == split_want
            # the flag changes nothing for text that is not gzip
            got = e.upload_fastx(data, 2, inflate=True)
            same_reads(got, want, "plain text under the flag")
            got.free()
        finally:
            want.free()
    finally:
        e.close()


def upload_other_batch_body(tmp_path):
    """smr_reads_upload_fastx_batch: batch 1 on the upload stream"""
    from test_gpu_fastx_device import same_reads, scan_text
    data = scan_text(True, 65)
    e = smr.Engine(0)
    try:
        want = e.upload_fastx(data, 1, batch=1)
        got = e.upload_fastx(deflate(data, 6), 1, batch=1, inflate=True)
        assert e.gunzip_info()["path"] == "device"
        same_reads(got, want, "batch 1")
        got.free()
        want.free()
    finally:
        e.close()


def upload_refusals_body(tmp_path):
    """a file zlib refuses, and irregular text in a good file: the code and the message of the call without the flag"""
    from test_gpu_fastx_device import scan_text
    e = smr.Engine(0)
    try:
        good, bad = refusal_blobs()
        bad["irregular text"] = deflate(scan_text(True, 65).replace(b"@7\n", b"\n@7\n"), 6)
        bad["no FASTX text"] = deflate(b"reads\n" * 10, 6)
        for k, (what, blob) in enumerate(bad.items()):
            path = os.path.join(str(tmp_path), "bad%d.fq.gz" % k)
            with open(path, "wb") as f:
                f.write(blob)
            seen = []
            for inflate in (False, True):
                try:
                    r = e.upload_fastx(path, 1, inflate=inflate)
                    seen.append((0, r.count, r.digest))
                    r.free()
                except smr.SmrError as x:
                    seen.append(str(x))
            assert seen[0] == seen[1], "%s: without the flag %r, with it %r" % (what, seen[0], seen[1])
            if what not in ("irregular text",):
                assert isinstance(seen[0], str), what
            ok = e.upload_fastx(deflate(scan_text(True, 64), 6), 1, inflate=True)
            assert ok.count == 64 and e.gunzip_info()["path"] == "device"
            ok.free()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ the amplicon fixture
def amplicon_body(n_bytes):
    """n_bytes = 0: the fixture as it is; else its first n_bytes of text, compressed by Python"""
    blob = open(AMPLICON, "rb").read()
    if n_bytes:
        blob = deflate(gzip.open(AMPLICON, "rb").read(n_bytes), 6)
    e = smr.Engine(0)
    try:
        for grain in GRAINS:
            on_device(e, blob, grain, "amplicon reads")
            print("amplicon reads, grain %d: %s" % (grain, e.gunzip_times()))
    finally:
        e.close()
