"""World-N worker for tests/test_gpu_split_p32.py (one process per rank, all on cuda:0, gloo for the
gathers): shard.sharded_compress of the file src across the ranks with MODEL_PARALLEL32 and split_p32
at split_bytes, which on rank 0 must equal the whole-file compress (every rank makes that one too);
then shard.sharded_decompress of the container across the ranks, each regenerating its range of
units on the P32 split kernel.  Rank 0 writes the file to dst and the container to dst + ".avrc"."""
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
            ctx.split_p32 = True
            ctx.split_bytes = int(split_bytes)
            avrc = ctx.compress(data, avr.MODEL_PARALLEL32)
            assert avr.seams_of_container(avrc)
            got = shard.sharded_compress(ctx, data, model=avr.MODEL_PARALLEL32, split_bytes=int(split_bytes),
                                         split_p32=True)
            assert got == avrc if dist.get_rank() == 0 else got is None
            out = shard.sharded_decompress(ctx, avrc)
            if dist.get_rank() == 0:
                Path(dst + ".avrc").write_bytes(got)
                Path(dst).write_bytes(out)
            else:
                assert out is None
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:4])
