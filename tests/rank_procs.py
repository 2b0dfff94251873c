"""Spawned processes that play the ranks of a process group in the tests, with bounded waits that end at the first failure.

A rank's target returns its result; a rank that raises reports the traceback through the queue and exits.  The parent stops waiting at the first
error report, or at the first rank process that has exited without a result, and kills whatever is still running: a failing rank costs the test
seconds, not its whole time limit."""
import queue
import socket
import time
import traceback


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(target, rank, world, port, out_q, args):
    try:
        value = target(rank, world, port, *args)
    except BaseException:
        out_q.put((rank, "error", traceback.format_exc()))
        raise
    out_q.put((rank, "ok", value))


def run_ranks(world, target, args=(), timeout=300.0):
    """target(rank, world, port, *args) in `world` spawned processes (one free port for the group); -> {rank: return value}.  Raises
    AssertionError with the failing rank's traceback as soon as a rank raises or dies, or when `timeout` seconds have passed."""
    import torch.multiprocessing as mp

    port = free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(target, r, world, port, q, tuple(args))) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    ok = False
    deadline = time.monotonic() + timeout

    def take(wait):
        rank, status, value = q.get(timeout=wait)
        if status == "error":
            raise AssertionError(f"rank {rank} of {world} raised:\n{value}")
        results[rank] = value

    try:
        while len(results) < world:
            try:
                take(0.5)
                continue
            except queue.Empty:
                pass
            gone = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode is not None and r not in results]
            if gone:
                try:
                    take(2.0)   # a result or an error report that was still in the pipe when the process ended
                    continue
                except queue.Empty:
                    r, code = gone[0]
                    raise AssertionError(f"rank {r} of {world} exited with code {code} without a result")
            if time.monotonic() > deadline:
                raise AssertionError(f"the {world} ranks did not finish within {timeout:.0f} s (results from ranks {sorted(results)})")
        ok = True
    finally:
        for p in procs:
            p.join(timeout=60 if ok else 2)
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    codes = [p.exitcode for p in procs]
    assert all(c == 0 for c in codes), f"rank exit codes {codes}"
    return results
