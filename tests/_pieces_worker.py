"""World-N worker for tests/test_gpu_pieces.py (one process per rank, all on cuda:0, gloo for the
gather): the file src compressed whole on every rank with the parallel model at split_bytes (the same
container everywhere, its long slices cut into pieces), then shard.sharded_decompress of it across
the ranks, each regenerating its range of units; rank 0 writes the file to dst."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(src: str, split_bytes: str, dst: str) -> None:
    import torch.distributed as dist

    import avrecode_amd as avr
    from avrecode_amd import shard

    dist.init_process_group("gloo")
    try:
        with avr.Context(0) as ctx:
            data = Path(src).read_bytes()
            ctx.split_bytes = int(split_bytes)
            avrc = ctx.compress(data, avr.MODEL_PARALLEL)
            assert avr.seams_of_container(avrc)
            out = shard.sharded_decompress(ctx, avrc)
            if dist.get_rank() == 0:
                Path(dst).write_bytes(out)
            else:
                assert out is None
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:4])
