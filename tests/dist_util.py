"""The multi-rank plumbing of the tests that run a worker on several ranks of one machine: a free TCP port for the rendezvous and one
launcher.  The workers themselves stay top-level functions of their test modules (a spawned child imports them by module name), and
so do the tests' own "every rank answered" assertions."""
import socket


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(worker, world, *args, spawned_manager=False):
    """Run worker(rank, world, port, ret, *args) on `world` spawned ranks with a fresh port and a manager dict `ret`, join them and
    return what the ranks left in `ret` as a plain dict.  spawned_manager: the manager's server is SPAWNED — a GPU test needs that,
    since a fork of its process would inherit the GPU state; the CPU tests use the plain one."""
    import torch.multiprocessing as mp
    with (mp.get_context("spawn").Manager() if spawned_manager else mp.Manager()) as mgr:
        ret = mgr.dict()
        mp.spawn(worker, args=(world, _free_port(), ret) + args, nprocs=world, join=True)
        return dict(ret)
