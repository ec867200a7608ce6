"""Streaming of text between a file and the device, chunk after chunk, with a thread at the file's end of it.

stream_chunks (DESIGN K20, K24) writes text that is formatted on the device: two device buffers, two pinned host buffers, a
copy stream and a writer thread.  Used by heatmap.write_matrix (plot_cnv's matrix files), by
cnv_regions.generate_cnv_region_reports (the CNV region reports) and by the .rds writer.

LineChunks (DESIGN K21, K22) reads a file in chunks of whole lines: two pinned host buffers and a reader thread.  Used by
device.read_table and device.read_mtx, which upload and parse chunk i while the thread reads chunk i + 1."""
from __future__ import annotations

import queue
import threading
import time

import numpy as np
import torch


def _pinned(n):
    return torch.empty(int(n), dtype=torch.uint8, pin_memory=True)


def _last_newline(arr, n):
    """Index of the last '\\n' of arr[:n], or -1."""
    hi = n
    while hi > 0:
        lo = max(0, hi - (1 << 16))
        hit = np.flatnonzero(arr[lo:hi] == 10)
        if hit.size:
            return lo + int(hit[-1])
        hi = lo
    return -1


class LineChunks:
    """The rest of the binary file `f` as chunks of whole lines of about `cap` bytes, read by a thread into two buffers in
    turn.  Within the `with` block get() blocks for the next chunk and returns (slot, buf, n) -- the first n bytes of the uint8
    CPU tensor buf, which the caller may read until it calls release(slot) --, or None at the end of the file.  Every chunk
    but the last ends in '\\n'; a chunk may be empty (the last one is when the file ends in '\\n' at a buffer's end).  What
    follows a chunk's last '\\n' is carried to the other buffer; a buffer doubles when one line is longer than it.
    stats["read_s"] gains the thread's seconds inside readinto and the newline search, stats["grown"], where the caller has
    that key, the doublings.  Leaving the block stops and joins the thread, and raises what the thread caught unless another
    exception is on its way; a caller whose device copies may still read a buffer synchronises before it leaves.
    alloc(n): a buffer of n bytes -- pinned memory, unless a test without a GPU says otherwise."""

    def __init__(self, f, cap, stats, alloc=_pinned):
        self._f, self._stats, self._alloc = f, stats, alloc
        self._pin = [alloc(cap), alloc(cap)]
        self._jobs, self._free = queue.Queue(), [threading.Semaphore(1), threading.Semaphore(1)]
        self._stop, self._failure = threading.Event(), []
        self.thread = threading.Thread(target=self._reader, daemon=True)

    def _reader(self):
        f, pin, free, stats = self._f, self._pin, self._free, self._stats
        try:
            slot, fill, eof = 0, 0, False
            free[0].acquire()
            while not eof and not self._stop.is_set():
                t0 = time.perf_counter()
                arr = pin[slot].numpy()
                total = fill
                while total < arr.size:
                    got = f.readinto(memoryview(arr)[total:])
                    if not got:
                        eof = True
                        break
                    total += got
                cut = total if eof else _last_newline(arr, total) + 1
                stats["read_s"] += time.perf_counter() - t0
                if cut == 0 and not eof:                          # one line is longer than the buffer: grow it and read on
                    bigger = self._alloc(2 * arr.size)
                    bigger[:total].copy_(pin[slot][:total])
                    pin[slot], fill = bigger, total
                    if "grown" in stats:
                        stats["grown"] += 1
                    continue
                self._jobs.put((slot, pin[slot], cut))            # only this thread writes a buffer, and only while it holds it
                nxt = 1 - slot
                free[nxt].acquire()                               # the chunk before this one has left that buffer
                tail = total - cut
                if pin[nxt].numel() <= tail:
                    pin[nxt] = self._alloc(2 * tail)
                if tail:
                    pin[nxt][:tail].copy_(pin[slot][cut:total])
                slot, fill = nxt, tail
        except Exception as exc:                                  # handed to the caller's thread by __exit__
            self._failure.append(exc)
        finally:
            self._jobs.put(None)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, exc_type, exc, tb):
        self._stop.set()
        for sem in self._free:
            sem.release()
        self.thread.join()
        if exc_type is None and self._failure:
            raise self._failure[0]

    def get(self):
        return self._jobs.get()

    def get_nowait(self):
        """The next chunk where the thread has it ready, else None: the end of the file is left for get()."""
        try:
            job = self._jobs.get_nowait()
        except queue.Empty:
            return None
        if job is None:
            self._jobs.put(None)
        return job

    def release(self, slot):
        self._free[slot].release()


def stream_chunks(f, cap, device, fill):
    """Writes chunk after chunk to the binary file `f`.  fill(buf) formats the next chunk into `buf`, a CUDA uint8 tensor of
    `cap` bytes on `device`, on the current stream, and returns its bytes; None ends the stream.  While fill() formats chunk
    i + 1, chunk i is copied to the host on a second stream and a writer thread hands chunk i - 1 to the file.  Returns a
    dict of counts and seconds (format_s: inside fill; copy_wait_s and write_s: the writer thread waiting for a copy and inside
    f.write; stall_s: this thread waiting for a free buffer; wall_s: all of it but the allocation of the buffers)."""
    stats = {"bytes": 0, "chunks": 0, "format_s": 0.0, "copy_wait_s": 0.0, "write_s": 0.0, "stall_s": 0.0}
    dev = [torch.empty(cap, dtype=torch.uint8, device=device) for _ in range(2)]
    pin = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    copy_stream = torch.cuda.Stream(device=device)
    jobs, free, failure = queue.Queue(), [threading.Semaphore(1), threading.Semaphore(1)], []
    t_start = time.perf_counter()

    def writer():
        while True:
            job = jobs.get()
            if job is None:
                return
            slot, nbytes, event = job
            try:
                if not failure:
                    t0 = time.perf_counter()
                    event.synchronize()
                    t1 = time.perf_counter()
                    f.write(memoryview(pin[slot].numpy())[:nbytes])
                    stats["copy_wait_s"] += t1 - t0
                    stats["write_s"] += time.perf_counter() - t1
            except Exception as exc:          # handed to the caller's thread below
                failure.append(exc)
            finally:
                free[slot].release()

    thread = threading.Thread(target=writer, daemon=True)
    thread.start()
    try:
        i = 0
        while not failure:
            slot = i % 2
            t0 = time.perf_counter()
            free[slot].acquire()               # chunk i - 2 has left this pair of buffers
            t1 = time.perf_counter()
            try:
                nbytes = fill(dev[slot])
            except Exception:
                free[slot].release()
                raise
            if nbytes is None:
                free[slot].release()
                break
            stats["stall_s"] += t1 - t0
            stats["format_s"] += time.perf_counter() - t1
            copy_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(copy_stream):
                pin[slot][:nbytes].copy_(dev[slot][:nbytes], non_blocking=True)
                event = torch.cuda.Event()
                event.record(copy_stream)
            jobs.put((slot, nbytes, event))
            i += 1
            stats["bytes"] += nbytes
            stats["chunks"] += 1
    finally:
        jobs.put(None)
        thread.join()
    if failure:
        raise failure[0]
    stats["wall_s"] = time.perf_counter() - t_start
    return stats
