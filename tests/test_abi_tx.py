"""The transmit-side extension of the C ABI (include/capsule_gpu_tx.h): its
cgtx_ declarations equal the binding's TX_EXPORTS, the library exports them,
and the host-only entry points and every call-level argument check behave as
the header says.  No GPU work: cgtx_build_batch checks its arguments before
it touches the context or the device, so the context here is a zeroed
stand-in (as in test_abi.test_host_register_takes_whole_pages_only)."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

from capsule_amd import _native as N
from capsule_amd import packets

ROOT = pathlib.Path(__file__).resolve().parents[1]
REC = np.dtype(N.HDR_RECORD_FIELDS)


def declared():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "capsule_gpu_tx.h").read_text(), flags=re.S)
    return set(re.findall(r"\b(cgtx_\w+)\s*\(", text))


def test_header_declares_what_binding_binds():
    assert declared() == set(N.TX_EXPORTS)
    assert len(N.TX_EXPORTS) == 4


def test_library_exports_the_extension():
    L = N.lib()
    for name in N.TX_EXPORTS:
        assert hasattr(L, name), name
    for path in (N.LIB_PATH, N.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        assert set(N.TX_EXPORTS) <= set(re.findall(r"\b(cgtx_\w+)\b", out)), path
    assert L.cgtx_abi_version() == N.TX_ABI_VERSION == 1
    assert L.cgpu_abi_version() == 6  # the receive side's version did not move


def test_header_says_why_it_is_separate():
    head = (ROOT / "include" / "capsule_gpu_tx.h").read_text().split("#ifndef")[0]
    for word in ("test_abi.py", "abi_check.c", "CGTX_ABI_VERSION", "TX_EXPORTS"):
        assert word in head, word


CHAINS = [(4, 17), (4, 6), (4, 1), (6, 17), (6, 6), (6, 58)]


@pytest.mark.parametrize("version,proto", CHAINS)
def test_hdr_defaults(version, proto):
    L = N.lib()
    rec = np.full(1, 0xFF, np.uint8).repeat(96).view(REC)
    assert L.cgtx_hdr_defaults(version, proto, rec.ctypes.data) == 0
    want = np.zeros(1, REC)
    want["version"], want["ttl"], want["protocol"] = version, 64, proto
    want["ihl"] = 5 if version == 4 else 0
    want["data_offset"] = 5 if proto == 6 else 0
    assert rec.tobytes() == want.tobytes()
    l4 = {17: "udp", 6: "tcp"}.get(proto, "icmp")
    assert packets.hdr_defaults(version, l4).tobytes() == want.tobytes()


@pytest.mark.parametrize("version,proto", [(4, 58), (6, 1), (5, 17), (0, 0), (4, 2), (6, 0), (4, 256 + 17)])
def test_hdr_defaults_rejects_other_pairs(version, proto):
    L = N.lib()
    rec = np.zeros(1, REC)
    assert L.cgtx_hdr_defaults(version, proto, rec.ctypes.data) == N.EINVAL
    assert L.cgpu_last_error() == N.EINVAL
    assert L.cgtx_hdr_defaults(4, 17, None) == N.EINVAL


def test_status_strings():
    L = N.lib()
    seen = set()
    for s, name in enumerate(N.BUILD_STATUS):
        text = L.cgtx_build_status_str(s)
        assert text and text != b"unknown status", name
        seen.add(text)
    assert len(seen) == 4
    assert L.cgtx_build_status_str(N.BUILD["OK"]) == b"ok"
    assert L.cgtx_build_status_str(N.BUILD["NO_ROOM"]) == b"buffer not resized"
    assert L.cgtx_build_status_str(4) == b"unknown status"
    assert L.cgtx_build_status_str(-1) == b"unknown status"


def _call(L, ctx, rec, n, pay, out, room=2048):
    return L.cgtx_build_batch(ctx, rec, n, ctypes.byref(pay) if pay is not None else None,
                              ctypes.byref(out) if out is not None else None, room, None)


def test_call_level_errors():
    """Every CGPU_EINVAL of the header, and n == 0; no address here is ever
    dereferenced (they are made-up device addresses)."""
    L = N.lib()
    ctx = ctypes.create_string_buffer(1 << 16)
    rec = ctypes.c_void_p(0x10000)

    def out(arena=0x100000, alen=1 << 16, off=0x200000, ln=0x300000, status=0):
        o = N.TxFramesOut()
        o.arena, o.arena_len, o.off, o.len, o.status = arena, alen, off, ln, status
        return o

    def pay(arena=0x800000, alen=1 << 16, off=0x900000, ln=0xA00000):
        p = N.TxPayload()
        p.arena, p.arena_len, p.off, p.len = arena, alen, off, ln
        return p

    bad = [
        (None, rec, 1, None, out(), 2048),                      # NULL ctx
        (ctx, None, 1, None, out(), 2048),                      # NULL rec
        (ctx, rec, 1, None, None, 2048),                        # NULL out
        (ctx, rec, 1, None, out(arena=0), 2048),                # NULL out->arena
        (ctx, rec, 1, None, out(off=0), 2048),                  # NULL out->off
        (ctx, rec, 1, None, out(ln=0), 2048),                   # NULL out->len
        (ctx, rec, (1 << 30), None, out(), 2048),               # n > CGPU_MAX_BATCH
        (ctx, rec, 1, None, out(), 0),                          # room == 0
        (ctx, rec, 1, None, out(), 65537),                      # room > 65536
        (ctx, rec, 1, None, out(alen=0xFFFF0001), 2048),        # out arena too long
        (ctx, rec, 1, pay(alen=0xFFFF0001), out(arena=1 << 40), 2048),  # payload arena too long
        (ctx, rec, 1, pay(off=0), out(), 2048),                 # payload arena without off
        (ctx, rec, 1, pay(ln=0), out(), 2048),                  # ... without len
        (ctx, rec, 1, pay(arena=0x100000 + 100), out(), 2048),  # ranges overlap (payload inside)
        (ctx, rec, 1, pay(arena=0x100000 - 10, alen=11), out(), 2048),  # overlap by one byte
        (ctx, rec, 0, None, None, 2048),                        # the checks come before n == 0
    ]
    for k, (c, r, n, p, o, room) in enumerate(bad):
        assert _call(L, c, r, n, p, o, room) == N.EINVAL, k
        assert L.cgpu_last_error() == N.EINVAL, k
    # n == 0 with valid arguments: 0, and no launch (the context is a stand-in)
    assert _call(L, ctx, rec, 0, None, out(), 2048) == 0
    assert L.cgpu_last_error() == 0
    assert _call(L, ctx, rec, 0, pay(), out(), 65536) == 0
    # ranges that only touch do not overlap; a NULL payload arena is "no payload"
    assert _call(L, ctx, rec, 0, pay(arena=0x100000 - 10, alen=10), out(), 1) == 0
    assert _call(L, ctx, rec, 0, pay(arena=0, off=0, ln=0), out(), 2048) == 0


def test_binding_structs_match_the_header():
    assert ctypes.sizeof(N.TxPayload) == 32 and ctypes.sizeof(N.TxFramesOut) == 40
    assert N.TxFramesOut.status.offset == 32 and N.TxPayload.len.offset == 24
    assert N.BUILD == {"OK": 0, "BAD_RECORD": 1, "NO_ROOM": 2, "BAD_PAYLOAD": 3}


def test_plain_c_consumer_compiles_and_links(tmp_path):
    exe = tmp_path / "abi_tx_check"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic",
                    f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c" / "abi_tx_check.c"),
                    f"-L{N.LIB_PATH.parent}", "-lcapsule_gpu",
                    f"-Wl,-rpath,{N.LIB_PATH.parent}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.startswith(f"abi tx ok: {len(N.TX_EXPORTS)} entry points, version 1")
