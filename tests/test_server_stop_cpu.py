"""ModelhubServer.stop() returns only once the engine loop has left, so a
caller may tear down what the loop uses (under expert parallelism: the
process group its lockstep collectives run on) right after it."""
import os
import uuid

import torch.distributed as dist
import torch.multiprocessing as mp


def test_stop_joins_engine_loop(tmp_path):
    from kukeon_amd.engine.config import EngineConfig, tiny_llama
    from kukeon_amd.models.llama import LlamaModel
    from kukeon_amd.serve.server import ModelhubClient, ModelhubServer
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=128, max_sessions=2, num_kv_blocks=64,
                        use_graphs=False)
    sock = str(tmp_path / "hub.sock")
    hub = ModelhubServer(LlamaModel(cfg, device="cpu"), cfg, ecfg, sock,
                         device="cpu")
    hub.start()
    c = ModelhubClient(sock, timeout=60)
    assert len(c.generate("s", [1, 2, 3], max_new_tokens=2,
                          temperature=0.0)["tokens"]) == 2
    c.close()
    assert hub._engine_thread.is_alive()
    hub.stop()
    assert not hub._engine_thread.is_alive()


def _worker(rank, world, port):
    """Rank 1 is done after one short request and stops at once; rank 0
    still has several turns to serve, which need rank 1's experts. Rank
    1's stop() has to keep its engine loop participating until rank 0 has
    voted stop too, and only then let the caller destroy the group."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from kukeon_amd import parallel
    parallel.init_expert_parallel(world)
    from kukeon_amd.engine.config import EngineConfig, tiny_mixtral
    from kukeon_amd.models.mixtral import MixtralModel
    from kukeon_amd.serve.server import ModelhubClient, ModelhubServer

    cfg = tiny_mixtral()
    ecfg = EngineConfig(max_model_len=128, max_sessions=4,
                        num_kv_blocks=64, use_graphs=False)
    sock = f"/tmp/mh-stop-{rank}-{uuid.uuid4().hex[:8]}.sock"
    hub = ModelhubServer(MixtralModel(cfg, device="cpu"), cfg, ecfg, sock,
                         device="cpu")
    hub.start()
    try:
        c = ModelhubClient(sock, timeout=60)
        if rank == 1:
            r = c.generate("s1", [5, 6, 7], max_new_tokens=2,
                           temperature=0.0)
            assert len(r["tokens"]) == 2
        else:
            for turn in range(8):
                r = c.generate("s0", [1 + turn, 2, 3], max_new_tokens=8,
                               temperature=0.0)
                assert len(r["tokens"]) == 8
        c.close()
    finally:
        hub.stop()
    assert not hub._engine_thread.is_alive()
    dist.destroy_process_group()


def test_ep_stop_keeps_serving_until_every_rank_stops():
    port = 30300 + (os.getpid() + 7) % 500
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)
