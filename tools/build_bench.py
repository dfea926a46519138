"""Kernel time of cgtx_build_batch (capsule_amd/csrc/build.hip), by device
events over many launches, with reconcile64 beside it for orientation.

  (a) syn-flood: n x 54-B Eth/IPv4/TCP SYN frames, no payload, 64-B slots
  (b) n x 256-B Eth/IPv4/UDP frames, the 214-B payload from a device arena
  (c) cgpu_reconcile over n x 64-B Eth/IPv4/UDP frames (bench.py's
      reconcile64 workload): it also touches every frame once each way

Every launch works on another copy of its inputs and outputs; the copies of
one case add up to more than twice the 256 MiB Infinity Cache, as in
bench.py.  Bytes are the algorithm's: the records, descriptors and payload
read, the frames, lengths and statuses written.  Prints one JSON line per
case; `share_of_8TBps` is against the 8 TB/s HBM figure DESIGN.md uses.

    python tools/build_bench.py [--n 1048576] [--launches 1000]
"""
import argparse
import ctypes
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from capsule_amd import _native as N  # noqa: E402
from capsule_amd import packets, synth  # noqa: E402

CACHE = 256 << 20
PEAK = 8e12


class BuildLauncher:
    """A cgtx_build_batch call with prebuilt ctypes arguments."""

    def __init__(self, ctx, rec, out_arena, out_off, pay=None, room=2048):
        n = rec.shape[0]
        self.len = torch.empty(n, dtype=torch.int16, device=rec.device)
        self.status = torch.empty(n, dtype=torch.uint8, device=rec.device)
        self._keep = (rec, out_arena, out_off, pay)
        self.fo = N.TxFramesOut()
        self.fo.arena, self.fo.arena_len = out_arena.data_ptr(), out_arena.numel()
        self.fo.off, self.fo.len, self.fo.status = out_off.data_ptr(), self.len.data_ptr(), self.status.data_ptr()
        self.pay = None
        if pay is not None:
            self.pay = N.TxPayload()
            self.pay.arena, self.pay.arena_len = pay.arena.data_ptr(), pay.arena.numel()
            self.pay.off, self.pay.len = pay.off.data_ptr(), pay.len.data_ptr()
        self._fn = ctx.L.cgtx_build_batch
        self._args = [ctx.handle, ctypes.c_void_p(rec.data_ptr()), n,
                      ctypes.byref(self.pay) if self.pay is not None else None,
                      ctypes.byref(self.fo), room,
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]

    def __call__(self):
        rc = self._fn(*self._args)
        if rc:
            N.check(rc, "cgtx_build_batch")


def timed(launchers, launches, warmup=20):
    for k in range(warmup):
        launchers[k % len(launchers)]()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(launches):
        launchers[k % len(launchers)]()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches  # us per launch


def report(name, us, rd, wr, copies, n, launches, extra=None):
    rate = (rd + wr) / (us * 1e-6)
    out = dict(case=name, n=n, launches=launches, copies=copies, us_per_launch=round(us, 2),
               bytes_read=rd, bytes_written=wr, bytes_per_s=round(rate, -9),
               share_of_8TBps=round(rate / PEAK, 4), device=torch.cuda.get_device_name(0))
    out.update(extra or {})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("build_bench: no GPU (a CPU run measures nothing)")
    n, dev = a.n, "cuda:0"
    ctx = packets.Context(0)

    def slots(slot):
        o = torch.arange(n, device=dev, dtype=torch.int64) * slot
        return torch.where(o >= 1 << 31, o - (1 << 32), o).to(torch.int32)

    # (a) syn-flood records: what batch.syn_flood hands to build()
    rec = packets.default_records(n, 4, "tcp", dev)
    packets.record_set(rec, "src_mac", b"\x02\x00\x00\x00\x00\x01")
    packets.record_set(rec, "dst_mac", b"\x02\x00\x00\xff\xff\xff")
    packets.record_set(rec, "dst_ip", bytes([10, 100, 1, 255]))
    packets.record_set(rec, "tcp_flags", 2)
    packets.record_set(rec, "seq_no", 1)
    packets.record_set(rec, "udp_length_or_window", 10)
    packets.record_set(rec, "dst_port", 80)
    ip = torch.arange(1, n + 1, device=dev, dtype=torch.int64) + (10 << 24)
    rec[:, 40:44] = torch.stack([(ip >> s) & 0xFF for s in (24, 16, 8, 0)], dim=1).to(torch.uint8)
    per = n * (96 + 64)
    copies = max(2, -(-2 * CACHE // per))
    off = slots(64)
    ls = [BuildLauncher(ctx, rec.clone(), torch.empty(n * 64, dtype=torch.uint8, device=dev), off)
          for _ in range(copies)]
    us = timed(ls, a.launches)
    assert int(ls[0].status.max()) == 0 and int(ls[0].len.min()) == 54
    report("build_syn_flood_54B", us, n * (96 + 4), n * (54 + 3), copies, n, a.launches)
    del ls

    # (b) 256-B IPv4/UDP frames, 214-B payloads from a device arena (256-B slots)
    rec = packets.default_records(n, 4, "udp", dev)
    packets.record_set(rec, "src_port", 1234)
    packets.record_set(rec, "dst_port", 5678)
    rec[:, 40:44] = torch.stack([(ip >> s) & 0xFF for s in (24, 16, 8, 0)], dim=1).to(torch.uint8)
    per = n * (96 + 256 + 256)
    copies = max(2, -(-2 * CACHE // per))
    off = slots(256)
    plen = torch.full((n,), 214, dtype=torch.int16, device=dev)
    ls = []
    for _ in range(copies):
        pay = packets.PacketBatch(torch.randint(0, 256, (n * 256,), dtype=torch.uint8, device=dev), off, plen)
        ls.append(BuildLauncher(ctx, rec.clone(), torch.empty(n * 256, dtype=torch.uint8, device=dev), off, pay))
    us = timed(ls, a.launches)
    assert int(ls[0].status.max()) == 0 and int(ls[0].len.min()) == 256
    report("build_udp_256B", us, n * (96 + 4 + 4 + 2 + 214), n * (256 + 3), copies, n, a.launches)
    del ls

    # (c) reconcile64, for orientation
    arena, o, ln = synth.uniform(n, seed=0)
    flags = N.F_ACCEPT_V4 | N.F_ACCEPT_UDP
    per = len(arena)
    copies = max(2, -(-2 * CACHE // per))
    ls = []
    for _ in range(copies):
        b = packets.PacketBatch.from_numpy(arena, o, ln, dev)
        meta = packets.parse(ctx, b, flags=flags).meta
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        ls.append(packets.ReconcileLauncher(ctx, b, meta, flags, "l4", None, st))
    us = timed(ls, a.launches)
    report("reconcile64", us, int(ln.astype(np.int64).sum()) + n * 10, n * (8 + 1), copies, n, a.launches,
           dict(note="reads every frame byte + descriptor + meta; writes UDP length + checksum, "
                     "IPv4 total_length + header checksum, status"))
    ctx.check()
    ctx.close()


if __name__ == "__main__":
    main()
