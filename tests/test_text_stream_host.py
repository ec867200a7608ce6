"""text_stream.LineChunks, the reader thread of device.read_table and device.read_mtx, on the host: io.BytesIO files and
buffers that are not pinned.  Every scenario runs in a thread of its own that is joined with a time limit, so a reader that
no longer ends fails the test."""
import io
import random
import threading

import pytest

torch = pytest.importorskip("torch")

from infercnv_amd.text_stream import LineChunks   # noqa: E402

JOIN_S = 30.0


def unpinned(n):
    return torch.empty(n, dtype=torch.uint8)


def within_limit(fn):
    """fn() on a thread that is joined with a time limit: its value, or its exception raised here."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as exc:
            box["raised"] = exc
    worker = threading.Thread(target=run, daemon=True)
    worker.start()
    worker.join(JOIN_S)
    assert not worker.is_alive(), "the scenario did not end"
    if "raised" in box:
        raise box["raised"]
    return box["value"]


def chunks_of(f, cap, stats=None):
    """The chunks of LineChunks over the binary file f, as bytes, and the stats dict."""
    stats = {"read_s": 0.0, "grown": 0} if stats is None else stats

    def consume():
        out = []
        with LineChunks(f, cap, stats, alloc=unpinned) as chunks:
            while True:
                job = chunks.get()
                if job is None:
                    break
                slot, buf, n = job
                out.append(buf.numpy()[:n].tobytes())
                chunks.release(slot)
        assert not chunks.thread.is_alive()
        return out
    return within_limit(consume), stats


def sizes(data, cap, stats=None):
    got, stats = chunks_of(io.BytesIO(data), cap, stats)
    assert b"".join(got) == data
    return [len(c) for c in got], stats


@pytest.mark.parametrize("cap", [64, 65, 128, 333, 4096])
def test_random_files_come_back_whole_in_chunks_of_whole_lines(cap):
    rng = random.Random(cap)
    for _ in range(40):
        lines = [bytes(rng.choice(b"abc \t0123456789.\r") for _ in range(rng.randint(0, 200))) for _ in range(rng.randint(0, 40))]
        for final_newline in (True, False):
            data = b"\n".join(lines) + (b"\n" if final_newline and lines else b"")
            got, stats = chunks_of(io.BytesIO(data), cap)
            assert b"".join(got) == data
            assert all(c and c.endswith(b"\n") for c in got[:-1])
            assert stats["read_s"] >= 0.0


def test_an_empty_file_is_one_empty_chunk():
    assert sizes(b"", 64)[0] == [0]


def test_a_file_that_ends_with_a_full_buffer_has_an_empty_last_chunk():
    line = b"x" * 63 + b"\n"
    assert sizes(line, 64)[0] == [64, 0]
    assert sizes(line + line, 64)[0] == [64, 64, 0]


def test_a_line_longer_than_the_buffer_grows_it():
    assert sizes(b"x" * 64 + b"\n" + b"y" * 10, 64)[0] == [75]
    _, stats = sizes(b"x" * 500 + b"\nab\n", 64)
    assert stats["grown"] == 3


def test_grown_is_counted_only_where_the_caller_has_the_key():
    _, stats = sizes(b"x" * 500 + b"\nab\n", 64, stats={"read_s": 0.0})
    assert set(stats) == {"read_s"}


class Marker(Exception):
    pass


def test_a_consumer_that_raises_sees_its_own_exception_and_the_thread_ends():
    seen = {}

    def consume():
        with LineChunks(io.BytesIO((b"x" * 63 + b"\n") * 100), 64, {"read_s": 0.0}, alloc=unpinned) as chunks:
            seen["chunks"] = chunks
            assert chunks.get() is not None                          # not released: the reader waits for a buffer
            raise Marker()
    with pytest.raises(Marker):
        within_limit(consume)
    seen["chunks"].thread.join(JOIN_S)
    assert not seen["chunks"].thread.is_alive()


class FailsOnThirdRead(io.BytesIO):
    calls = 0

    def readinto(self, b):
        self.calls += 1
        if self.calls == 3:
            raise OSError("the third read fails")
        return super().readinto(b)


def test_a_failure_of_the_reader_is_raised_when_the_block_is_left():
    f = FailsOnThirdRead((b"x" * 63 + b"\n") * 100)
    with pytest.raises(OSError, match="the third read fails"):
        chunks_of(f, 64)
    assert f.calls == 3


def test_get_nowait_leaves_the_end_of_the_file_for_get():
    def consume():
        with LineChunks(io.BytesIO(b"ab\n"), 64, {"read_s": 0.0}, alloc=unpinned) as chunks:
            slot, buf, n = chunks.get()
            assert buf.numpy()[:n].tobytes() == b"ab\n"
            chunks.release(slot)
            chunks.thread.join(JOIN_S)                               # the file is read: the end is on the queue
            assert not chunks.thread.is_alive()
            return chunks.get_nowait(), chunks.get_nowait(), chunks.get()
    assert within_limit(consume) == (None, None, None)
