"""World-N worker for tests/test_gpu_checksum.py (one process per rank, all on cuda:0, gloo for the
gathers): shard.sharded_compress of the file src with checksums, which on rank 0 must equal the
whole-file compress with Context.checksums on (every rank makes that one too); shard.sharded_decompress
of that container and of the same file's container split at 1024, each rank computing its slices' or
units' CRCs on the device; and a damaged container, which must raise on rank 0 with ERR_CHECKSUM.
Rank 0 writes the two restored files to dst and dst + ".split"."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(src: str, dst: str) -> None:
    import torch.distributed as dist

    import avrecode_amd as avr
    from avrecode_amd import shard

    dist.init_process_group("gloo")
    try:
        with avr.Context(0) as ctx:
            data = Path(src).read_bytes()
            ctx.checksums = True
            ctx.split_bytes = 0
            plain = ctx.compress(data, avr.MODEL_PARALLEL)
            ctx.split_bytes = 1024
            split = ctx.compress(data, avr.MODEL_PARALLEL)
            assert avr.file_crc_of_container(plain) is not None and avr.seams_of_container(split)
            rank0 = dist.get_rank() == 0
            got = shard.sharded_compress(ctx, data, checksums=True)
            assert got == plain if rank0 else got is None
            got = shard.sharded_compress(ctx, data, split_bytes=1024, checksums=True)
            assert got == split if rank0 else got is None
            out = shard.sharded_decompress(ctx, plain)
            out_split = shard.sharded_decompress(ctx, split)
            if rank0:
                Path(dst).write_bytes(out)
                Path(dst + ".split").write_bytes(out_split)
            else:
                assert out is None and out_split is None
            # one bit of a coded block's stream: whatever it decodes to, rank 0 does not return it
            blocks = [b for b in avr.describe_container(plain)[0]["blocks"] if "cabac" in b]
            c = bytes.fromhex(blocks[1]["cabac"])
            damaged = bytearray(plain)
            damaged[plain.find(c) + len(c) // 2] ^= 0x10
            try:
                bad = shard.sharded_decompress(ctx, bytes(damaged))
                assert not rank0 and bad is None
            except avr.AvrError as e:
                assert rank0 and e.code in (avr.ERR_CHECKSUM, -3), e
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:3])
