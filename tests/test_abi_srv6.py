"""The segment-routing extension of the C ABI (include/capsule_gpu_srv6.h):
its cgsr_ declarations equal the binding's SR_EXPORTS, both libraries export
them, the two pinned surfaces did not move, and every call-level argument
check behaves as the header says.  No GPU work: cgsr_apply checks its
arguments before it touches the context or the device, so the context here
is a zeroed stand-in (as in test_abi_tx.py)."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np

from capsule_amd import _native as N

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "capsule_gpu_srv6.h"


def declared(prefix):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"\b(%s_\w+)\s*\(" % prefix, text))


def test_header_declares_what_binding_binds():
    assert declared("cgsr") == set(N.SR_EXPORTS)
    assert len(N.SR_EXPORTS) == 3
    assert not declared("cgpu") and not declared("cgtx")


def test_library_exports_the_extension():
    L = N.lib()
    for name in N.SR_EXPORTS:
        assert hasattr(L, name), name
    for path in (N.LIB_PATH, N.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        assert set(N.SR_EXPORTS) <= set(re.findall(r"\b(cgsr_\w+)\b", out)), path
    assert L.cgsr_abi_version() == N.SR_ABI_VERSION == 1
    assert L.cgpu_abi_version() == 6 and L.cgtx_abi_version() == 1  # neither moved


def test_header_says_why_it_is_separate():
    head = HEADER.read_text().split("#ifndef")[0]
    for word in ("test_abi.py", "test_abi_tx.py", "abi_check.c", "CGSR_ABI_VERSION", "SR_EXPORTS"):
        assert word in head, word


def test_status_strings():
    L = N.lib()
    seen = set()
    for s in list(range(len(N.PKT_STATUS))) + sorted(N.SR_STATUS.values()):
        text = L.cgsr_status_str(s)
        assert text and text != b"unknown status", s
        seen.add(text)
    assert len(seen) == len(N.PKT_STATUS) + len(N.SR_STATUS)
    for s, name in enumerate(N.PKT_STATUS):
        assert L.cgsr_status_str(s) == L.cgpu_pkt_status_str(s), name
    assert L.cgsr_status_str(N.SR_STATUS["NOT_ROUTING"]) == b"not an IPv6 routing packet."
    for s in (-1, 20, 63, 69, 255, 256):
        assert L.cgsr_status_str(s) == b"unknown status", s
    assert sorted(N.SR_STATUS.values()) == [64, 65, 66, 67, 68]


def test_binding_structs_match_the_header():
    assert ctypes.sizeof(N.SrPolicies) == 32
    assert N.SrPolicies.n_policies.offset == 8 and N.SrPolicies.segments.offset == 16
    assert N.SrPolicies.n_segments_total.offset == 24
    dt = np.dtype(N.SR_POLICY_FIELDS)
    assert dt.itemsize == N.SR_POLICY_SIZE == 16
    assert [dt.fields[k][1] for k in ("seg_first", "n_segments", "segments_left", "tag", "flags")] == \
        [0, 4, 5, 6, 8]
    assert N.SR_OP == {"NONE": 0, "ENCAP": 1, "SET": 2, "END": 3, "DECAP": 4}


def test_call_level_errors():
    """Every CGPU_EINVAL of the header, and n == 0; no address here is ever
    dereferenced (they are made-up device addresses)."""
    L = N.lib()
    ctx = ctypes.create_string_buffer(1 << 16)

    def inb(arena=0x800000, alen=1 << 16, off=0x900000, ln=0xA00000, n=1):
        b = N.Batch()
        b.arena, b.arena_len, b.off, b.len, b.n = arena, alen, off, ln, n
        return b

    def pol(policy=0xB00000, n=4, segments=0xC00000, total=16):
        p = N.SrPolicies()
        p.policy, p.n_policies, p.segments, p.n_segments_total = policy, n, segments, total
        return p

    base = dict(ctx=ctx, inb=inb(), op=0x10000, pidx=0x20000, pol=pol(), flags=0, room=2048,
                out=0x100000, olen=1 << 16, ooff=0x200000, oln=0x300000, st=0x400000)

    def call(**kw):
        a = dict(base, **kw)
        return L.cgsr_apply(a["ctx"], ctypes.byref(a["inb"]) if a["inb"] is not None else None,
                            a["op"], a["pidx"],
                            ctypes.byref(a["pol"]) if a["pol"] is not None else None, a["flags"],
                            a["room"], a["out"], a["olen"], a["ooff"], a["oln"], a["st"], None)

    bad = [
        dict(ctx=None), dict(inb=None), dict(inb=inb(arena=0)), dict(inb=inb(off=0)),
        dict(inb=inb(ln=0)), dict(op=None), dict(out=None), dict(ooff=None), dict(oln=None),
        dict(pol=None), dict(pol=pol(policy=0)), dict(pol=pol(segments=0)),
        dict(inb=inb(n=1 << 30)), dict(room=0), dict(room=65537),
        dict(inb=inb(alen=0xFFFF0001), out=1 << 40), dict(olen=0xFFFF0001, inb=inb(arena=1 << 40)),
        dict(pol=pol(total=0x0FFF0001)),
        dict(inb=inb(arena=0x100000 + 100)),             # ranges overlap (in inside out)
        dict(inb=inb(arena=0x100000 - 10, alen=11)),     # overlap by one byte
        dict(inb=inb(n=0), out=None),                    # the checks come before n == 0
        dict(inb=inb(n=0), room=0),
    ]
    for k, kw in enumerate(bad):
        assert call(**kw) == N.EINVAL, k
        assert L.cgpu_last_error() == N.EINVAL, k
    # n == 0 with valid arguments: 0, and no launch (the context is a stand-in)
    assert call(inb=inb(n=0)) == 0
    assert L.cgpu_last_error() == 0
    assert call(inb=inb(n=0), room=65536, st=None) == 0
    # no policy_idx: pol may be NULL; ranges that only touch do not overlap
    assert call(inb=inb(n=0), pidx=None, pol=None) == 0
    assert call(inb=inb(n=0, arena=0x100000 - 10, alen=10), room=1) == 0


def test_plain_c_consumer_compiles_and_links(tmp_path):
    exe = tmp_path / "abi_srv6_check"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic",
                    f"-I{ROOT / 'include'}", str(ROOT / "tests" / "c" / "abi_srv6_check.c"),
                    f"-L{N.LIB_PATH.parent}", "-lcapsule_gpu",
                    f"-Wl,-rpath,{N.LIB_PATH.parent}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stdout.startswith(f"abi srv6 ok: {len(N.SR_EXPORTS)} entry points, version 1")
