"""World-N worker for tests/test_gpu_split_compress.py (one process per rank, all on cuda:0, gloo for
the gathers): shard.sharded_compress of the file src across the ranks with the parallel model at
split_bytes -- each rank's long slices through the split walk, their pieces checked on the device,
the seams fields gathered after the re-coded bytes; rank 0 writes the container to dst."""
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
            out = shard.sharded_compress(ctx, data, split_bytes=int(split_bytes))
            if dist.get_rank() == 0:
                assert avr.seams_of_container(out)
                Path(dst).write_bytes(out)
            else:
                assert out is None
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:4])
