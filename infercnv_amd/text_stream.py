"""Streaming of text that is formatted on the device into a file (DESIGN K20, K24): two device buffers, two pinned host
buffers, a copy stream and a writer thread.  Used by heatmap.write_matrix (plot_cnv's matrix files) and by
cnv_regions.generate_cnv_region_reports (the CNV region reports)."""
from __future__ import annotations

import queue
import threading
import time

import torch


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
