"""CPU: the block-kernel launcher's decisions (plan_run in libcoolmic-dsp_amd/csrc/k_block.hip) -- which kernel
serves a run, its tiles and grid, 1 or 4 waves per workgroup, the 2^31 refusal and which launches carry the
completion flag.  Every expected value below was recorded from the launcher as it stood before plan_run (commit
597c3ad, the macro ladders of launch_run), so these rules are the ones the kernels were measured under."""
import pytest

PCM, F32, VU = 1, 2, 4
CHANNELS = (1, 2, 3, 4, 5, 6, 8, 12, 16)

FORMS = {    # (channels, io, identity maps): (family, C, U, NW, MAP, STAGE, chunks, W, rows per tile) at 4096 x 65536
    (1, PCM, 1): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, PCM, 0): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, F32, 1): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, F32, 0): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, PCM | F32, 1): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, PCM | F32, 0): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, VU, 1): ('fast_ro', 1, 16, 1, 0, 0, 8, 0, 0),
    (1, VU, 0): ('fast_ro', 1, 16, 1, 0, 0, 8, 0, 0),
    (1, PCM | VU, 1): ('fast', 1, 4, 4, 0, 0, 32, 0, 0),
    (1, PCM | VU, 0): ('fast', 1, 4, 4, 0, 0, 32, 0, 0),
    (1, F32 | VU, 1): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, F32 | VU, 0): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, PCM | F32 | VU, 1): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (1, PCM | F32 | VU, 0): ('fast', 1, 4, 1, 0, 0, 32, 0, 0),
    (2, PCM, 1): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, PCM, 0): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, F32, 1): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, F32, 0): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, PCM | F32, 1): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, PCM | F32, 0): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, VU, 1): ('fast_ro', 2, 16, 1, 0, 0, 16, 0, 0),
    (2, VU, 0): ('fast_ro', 2, 16, 1, 0, 0, 16, 0, 0),
    (2, PCM | VU, 1): ('fast', 2, 4, 4, 0, 0, 64, 0, 0),
    (2, PCM | VU, 0): ('fast', 2, 4, 4, 0, 0, 64, 0, 0),
    (2, F32 | VU, 1): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, F32 | VU, 0): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, PCM | F32 | VU, 1): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (2, PCM | F32 | VU, 0): ('fast', 2, 4, 1, 0, 0, 64, 0, 0),
    (3, PCM, 1): ('rows', 0, 0, 1, 0, 0, 49, 63, 8),
    (3, PCM, 0): ('rows', 0, 0, 1, 1, 0, 25, 63, 16),
    (3, F32, 1): ('rows', 0, 0, 1, 0, 1, 49, 63, 8),
    (3, F32, 0): ('rows', 0, 0, 1, 1, 1, 25, 63, 16),
    (3, PCM | F32, 1): ('rows', 0, 0, 1, 0, 1, 49, 63, 8),
    (3, PCM | F32, 0): ('rows', 0, 0, 1, 1, 1, 25, 63, 16),
    (3, VU, 1): ('rows', 0, 0, 1, 0, 0, 7, 63, 56),
    (3, VU, 0): ('rows', 0, 0, 1, 1, 0, 7, 63, 56),
    (3, PCM | VU, 1): ('rows', 0, 0, 1, 0, 0, 49, 63, 8),
    (3, PCM | VU, 0): ('rows', 0, 0, 1, 1, 0, 25, 63, 16),
    (3, F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 49, 63, 8),
    (3, F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 25, 63, 16),
    (3, PCM | F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 49, 63, 8),
    (3, PCM | F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 25, 63, 16),
    (4, PCM, 1): ('wide', 4, 8, 1, 0, 0, 64, 0, 0),
    (4, PCM, 0): ('rows', 0, 0, 1, 1, 0, 16, 64, 32),
    (4, F32, 1): ('rows', 0, 0, 1, 0, 1, 16, 64, 32),
    (4, F32, 0): ('rows', 0, 0, 1, 1, 1, 16, 64, 32),
    (4, PCM | F32, 1): ('rows', 0, 0, 1, 0, 1, 16, 64, 32),
    (4, PCM | F32, 0): ('rows', 0, 0, 1, 1, 1, 16, 64, 32),
    (4, VU, 1): ('rows', 0, 0, 1, 0, 0, 8, 64, 64),
    (4, VU, 0): ('rows', 0, 0, 1, 1, 0, 8, 64, 64),
    (4, PCM | VU, 1): ('wide', 4, 8, 1, 0, 0, 64, 0, 0),
    (4, PCM | VU, 0): ('rows', 0, 0, 1, 1, 0, 16, 64, 32),
    (4, F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 16, 64, 32),
    (4, F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 16, 64, 32),
    (4, PCM | F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 16, 64, 32),
    (4, PCM | F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 16, 64, 32),
    (5, PCM, 1): ('rows', 0, 0, 1, 0, 0, 86, 60, 8),
    (5, PCM, 0): ('rows', 0, 0, 1, 1, 0, 43, 60, 16),
    (5, F32, 1): ('rows', 0, 0, 1, 0, 1, 86, 60, 8),
    (5, F32, 0): ('rows', 0, 0, 1, 1, 1, 43, 60, 16),
    (5, PCM | F32, 1): ('rows', 0, 0, 1, 0, 1, 86, 60, 8),
    (5, PCM | F32, 0): ('rows', 0, 0, 1, 1, 1, 43, 60, 16),
    (5, VU, 1): ('rows', 0, 0, 1, 0, 0, 11, 60, 64),
    (5, VU, 0): ('rows', 0, 0, 1, 1, 0, 11, 60, 64),
    (5, PCM | VU, 1): ('rows', 0, 0, 1, 0, 0, 86, 60, 8),
    (5, PCM | VU, 0): ('rows', 0, 0, 1, 1, 0, 43, 60, 16),
    (5, F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 86, 60, 8),
    (5, F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 43, 60, 16),
    (5, PCM | F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 86, 60, 8),
    (5, PCM | F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 43, 60, 16),
    (6, PCM, 1): ('rows', 0, 0, 1, 0, 0, 98, 63, 8),
    (6, PCM, 0): ('rows', 0, 0, 1, 1, 0, 49, 63, 16),
    (6, F32, 1): ('rows', 0, 0, 1, 0, 1, 98, 63, 8),
    (6, F32, 0): ('rows', 0, 0, 1, 1, 1, 49, 63, 16),
    (6, PCM | F32, 1): ('rows', 0, 0, 1, 0, 1, 98, 63, 8),
    (6, PCM | F32, 0): ('rows', 0, 0, 1, 1, 1, 49, 63, 16),
    (6, VU, 1): ('rows', 0, 0, 1, 0, 0, 13, 63, 64),
    (6, VU, 0): ('rows', 0, 0, 1, 1, 0, 13, 63, 64),
    (6, PCM | VU, 1): ('rows', 0, 0, 1, 0, 0, 98, 63, 8),
    (6, PCM | VU, 0): ('rows', 0, 0, 1, 1, 0, 49, 63, 16),
    (6, F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 98, 63, 8),
    (6, F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 49, 63, 16),
    (6, PCM | F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 98, 63, 8),
    (6, PCM | F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 49, 63, 16),
    (8, PCM, 1): ('wide', 8, 8, 1, 0, 0, 128, 0, 0),
    (8, PCM, 0): ('rows', 0, 0, 1, 1, 0, 32, 64, 32),
    (8, F32, 1): ('wide', 8, 8, 1, 0, 0, 128, 0, 0),
    (8, F32, 0): ('rows', 0, 0, 1, 1, 1, 32, 64, 32),
    (8, PCM | F32, 1): ('wide', 8, 8, 1, 0, 0, 128, 0, 0),
    (8, PCM | F32, 0): ('rows', 0, 0, 1, 1, 1, 32, 64, 32),
    (8, VU, 1): ('rows', 0, 0, 1, 0, 0, 16, 64, 64),
    (8, VU, 0): ('rows', 0, 0, 1, 1, 0, 16, 64, 64),
    (8, PCM | VU, 1): ('wide', 8, 8, 1, 0, 0, 128, 0, 0),
    (8, PCM | VU, 0): ('rows', 0, 0, 1, 1, 0, 32, 64, 32),
    (8, F32 | VU, 1): ('wide', 8, 8, 1, 0, 0, 128, 0, 0),
    (8, F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 32, 64, 32),
    (8, PCM | F32 | VU, 1): ('wide', 8, 8, 1, 0, 0, 128, 0, 0),
    (8, PCM | F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 32, 64, 32),
    (12, PCM, 1): ('rows', 0, 0, 1, 0, 0, 196, 63, 8),
    (12, PCM, 0): ('rows', 0, 0, 1, 1, 0, 98, 63, 16),
    (12, F32, 1): ('rows', 0, 0, 1, 0, 1, 196, 63, 8),
    (12, F32, 0): ('rows', 0, 0, 1, 1, 1, 98, 63, 16),
    (12, PCM | F32, 1): ('rows', 0, 0, 1, 0, 1, 196, 63, 8),
    (12, PCM | F32, 0): ('rows', 0, 0, 1, 1, 1, 98, 63, 16),
    (12, VU, 1): ('rows', 0, 0, 1, 0, 0, 25, 63, 64),
    (12, VU, 0): ('rows', 0, 0, 1, 1, 0, 25, 63, 64),
    (12, PCM | VU, 1): ('rows', 0, 0, 1, 0, 0, 196, 63, 8),
    (12, PCM | VU, 0): ('rows', 0, 0, 1, 1, 0, 98, 63, 16),
    (12, F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 196, 63, 8),
    (12, F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 98, 63, 16),
    (12, PCM | F32 | VU, 1): ('rows', 0, 0, 1, 0, 1, 196, 63, 8),
    (12, PCM | F32 | VU, 0): ('rows', 0, 0, 1, 1, 1, 98, 63, 16),
    (16, PCM, 1): ('rows', 0, 0, 1, 0, 0, 256, 64, 8),
    (16, PCM, 0): ('rows', 0, 0, 1, 1, 0, 128, 64, 16),
    (16, F32, 1): ('rows', 0, 0, 1, 0, 0, 256, 64, 8),
    (16, F32, 0): ('rows', 0, 0, 1, 1, 0, 128, 64, 16),
    (16, PCM | F32, 1): ('rows', 0, 0, 1, 0, 0, 256, 64, 8),
    (16, PCM | F32, 0): ('rows', 0, 0, 1, 1, 0, 128, 64, 16),
    (16, VU, 1): ('rows', 0, 0, 1, 0, 0, 32, 64, 64),
    (16, VU, 0): ('rows', 0, 0, 1, 1, 0, 32, 64, 64),
    (16, PCM | VU, 1): ('rows', 0, 0, 1, 0, 0, 256, 64, 8),
    (16, PCM | VU, 0): ('rows', 0, 0, 1, 1, 0, 128, 64, 16),
    (16, F32 | VU, 1): ('rows', 0, 0, 1, 0, 0, 256, 64, 8),
    (16, F32 | VU, 0): ('rows', 0, 0, 1, 1, 0, 128, 64, 16),
    (16, PCM | F32 | VU, 1): ('rows', 0, 0, 1, 0, 0, 256, 64, 8),
    (16, PCM | F32 | VU, 0): ('rows', 0, 0, 1, 1, 0, 128, 64, 16),
}
TILES = {    # (channels, io, frames) of one stream: (chunks, workgroups, threads, rows per tile, flag kept)
    # 1 channel, PCM | VU: fast, a tile of 2048 frames
    (1, PCM | VU, 1): (1, 1, 64, 0, 1),
    (1, PCM | VU, 2047): (1, 1, 64, 0, 1),
    (1, PCM | VU, 2048): (1, 1, 64, 0, 1),
    (1, PCM | VU, 2049): (2, 2, 64, 0, 0),
    (1, PCM | VU, 4096): (2, 2, 64, 0, 0),
    (1, PCM | VU, 4097): (3, 1, 256, 0, 1),
    (1, PCM | VU, 6143): (3, 1, 256, 0, 1),
    (1, PCM | VU, 6144): (3, 1, 256, 0, 1),
    (1, PCM | VU, 16384): (8, 2, 256, 0, 0),
    (1, PCM | VU, 65536): (32, 8, 256, 0, 0),
    # 1 channel, VU: fast_ro, a tile of 8192 frames
    (1, VU, 1): (1, 1, 64, 0, 1),
    (1, VU, 8191): (1, 1, 64, 0, 1),
    (1, VU, 8192): (1, 1, 64, 0, 1),
    (1, VU, 8193): (2, 2, 64, 0, 0),
    (1, VU, 16384): (2, 2, 64, 0, 0),
    (1, VU, 16385): (3, 3, 64, 0, 0),
    (1, VU, 24575): (3, 3, 64, 0, 0),
    (1, VU, 24576): (3, 3, 64, 0, 0),
    (1, VU, 65536): (8, 8, 64, 0, 0),
    # 2 channels, PCM | VU: fast, a tile of 1024 frames
    (2, PCM | VU, 1): (1, 1, 64, 0, 1),
    (2, PCM | VU, 1023): (1, 1, 64, 0, 1),
    (2, PCM | VU, 1024): (1, 1, 64, 0, 1),
    (2, PCM | VU, 1025): (2, 2, 64, 0, 0),
    (2, PCM | VU, 2048): (2, 2, 64, 0, 0),
    (2, PCM | VU, 2049): (3, 1, 256, 0, 1),
    (2, PCM | VU, 3071): (3, 1, 256, 0, 1),
    (2, PCM | VU, 3072): (3, 1, 256, 0, 1),
    (2, PCM | VU, 16384): (16, 4, 256, 0, 0),
    (2, PCM | VU, 65536): (64, 16, 256, 0, 0),
    # 2 channels, VU: fast_ro, a tile of 4096 frames
    (2, VU, 1): (1, 1, 64, 0, 1),
    (2, VU, 4095): (1, 1, 64, 0, 1),
    (2, VU, 4096): (1, 1, 64, 0, 1),
    (2, VU, 4097): (2, 2, 64, 0, 0),
    (2, VU, 8192): (2, 2, 64, 0, 0),
    (2, VU, 8193): (3, 3, 64, 0, 0),
    (2, VU, 12287): (3, 3, 64, 0, 0),
    (2, VU, 12288): (3, 3, 64, 0, 0),
    (2, VU, 16384): (4, 4, 64, 0, 0),
    (2, VU, 65536): (16, 16, 64, 0, 0),
    # 3 channels, PCM | VU: rows, a tile of 1344 frames
    (3, PCM | VU, 1): (1, 1, 64, 8, 1),
    (3, PCM | VU, 1343): (1, 1, 64, 8, 1),
    (3, PCM | VU, 1344): (1, 1, 64, 8, 1),
    (3, PCM | VU, 1345): (2, 2, 64, 8, 0),
    (3, PCM | VU, 2688): (2, 2, 64, 8, 0),
    (3, PCM | VU, 2689): (3, 3, 64, 8, 0),
    (3, PCM | VU, 4031): (3, 3, 64, 8, 0),
    (3, PCM | VU, 4032): (3, 3, 64, 8, 0),
    (3, PCM | VU, 16384): (13, 13, 64, 8, 0),
    (3, PCM | VU, 65536): (49, 49, 64, 8, 0),
    # 3 channels, VU: rows, a tile of 10752 frames
    (3, VU, 1): (1, 1, 64, 4, 1),
    (3, VU, 10751): (1, 1, 64, 64, 1),
    (3, VU, 10752): (1, 1, 64, 64, 1),
    (3, VU, 10753): (2, 2, 64, 36, 0),
    (3, VU, 16384): (2, 2, 64, 52, 0),
    (3, VU, 21504): (2, 2, 64, 64, 0),
    (3, VU, 21505): (3, 3, 64, 44, 0),
    (3, VU, 32255): (3, 3, 64, 64, 0),
    (3, VU, 32256): (3, 3, 64, 64, 0),
    (3, VU, 65536): (7, 7, 64, 56, 0),
    # 4 channels, PCM | VU: wide, a tile of 1024 frames
    (4, PCM | VU, 1): (1, 1, 64, 0, 1),
    (4, PCM | VU, 1023): (1, 1, 64, 0, 1),
    (4, PCM | VU, 1024): (1, 1, 64, 0, 1),
    (4, PCM | VU, 1025): (2, 2, 64, 0, 0),
    (4, PCM | VU, 2048): (2, 2, 64, 0, 0),
    (4, PCM | VU, 2049): (3, 3, 64, 0, 0),
    (4, PCM | VU, 3071): (3, 3, 64, 0, 0),
    (4, PCM | VU, 3072): (3, 3, 64, 0, 0),
    (4, PCM | VU, 16384): (16, 16, 64, 0, 0),
    (4, PCM | VU, 65536): (64, 64, 64, 0, 0),
    # 4 channels, VU: rows, a tile of 8192 frames
    (4, VU, 1): (1, 1, 64, 4, 1),
    (4, VU, 8191): (1, 1, 64, 64, 1),
    (4, VU, 8192): (1, 1, 64, 64, 1),
    (4, VU, 8193): (2, 2, 64, 36, 0),
    (4, VU, 16384): (2, 2, 64, 64, 0),
    (4, VU, 16385): (3, 3, 64, 44, 0),
    (4, VU, 24575): (3, 3, 64, 64, 0),
    (4, VU, 24576): (3, 3, 64, 64, 0),
    (4, VU, 65536): (8, 8, 64, 64, 0),
    # 5 channels, PCM | VU: rows, a tile of 768 frames
    (5, PCM | VU, 1): (1, 1, 64, 8, 1),
    (5, PCM | VU, 767): (1, 1, 64, 8, 1),
    (5, PCM | VU, 768): (1, 1, 64, 8, 1),
    (5, PCM | VU, 769): (2, 2, 64, 8, 0),
    (5, PCM | VU, 1536): (2, 2, 64, 8, 0),
    (5, PCM | VU, 1537): (3, 3, 64, 8, 0),
    (5, PCM | VU, 2303): (3, 3, 64, 8, 0),
    (5, PCM | VU, 2304): (3, 3, 64, 8, 0),
    (5, PCM | VU, 16384): (22, 22, 64, 8, 0),
    (5, PCM | VU, 65536): (86, 86, 64, 8, 0),
    # 5 channels, VU: rows, a tile of 6144 frames
    (5, VU, 1): (1, 1, 64, 4, 1),
    (5, VU, 6143): (1, 1, 64, 64, 1),
    (5, VU, 6144): (1, 1, 64, 64, 1),
    (5, VU, 6145): (2, 2, 64, 36, 0),
    (5, VU, 12288): (2, 2, 64, 64, 0),
    (5, VU, 12289): (3, 3, 64, 44, 0),
    (5, VU, 16384): (3, 3, 64, 60, 0),
    (5, VU, 18431): (3, 3, 64, 64, 0),
    (5, VU, 18432): (3, 3, 64, 64, 0),
    (5, VU, 65536): (11, 11, 64, 64, 0),
    # 6 channels, PCM | VU: rows, a tile of 672 frames
    (6, PCM | VU, 1): (1, 1, 64, 8, 1),
    (6, PCM | VU, 671): (1, 1, 64, 8, 1),
    (6, PCM | VU, 672): (1, 1, 64, 8, 1),
    (6, PCM | VU, 673): (2, 2, 64, 8, 0),
    (6, PCM | VU, 1344): (2, 2, 64, 8, 0),
    (6, PCM | VU, 1345): (3, 3, 64, 8, 0),
    (6, PCM | VU, 2015): (3, 3, 64, 8, 0),
    (6, PCM | VU, 2016): (3, 3, 64, 8, 0),
    (6, PCM | VU, 16384): (25, 25, 64, 8, 0),
    (6, PCM | VU, 65536): (98, 98, 64, 8, 0),
    # 6 channels, VU: rows, a tile of 5376 frames
    (6, VU, 1): (1, 1, 64, 4, 1),
    (6, VU, 5375): (1, 1, 64, 64, 1),
    (6, VU, 5376): (1, 1, 64, 64, 1),
    (6, VU, 5377): (2, 2, 64, 36, 0),
    (6, VU, 10752): (2, 2, 64, 64, 0),
    (6, VU, 10753): (3, 3, 64, 44, 0),
    (6, VU, 16127): (3, 3, 64, 64, 0),
    (6, VU, 16128): (3, 3, 64, 64, 0),
    (6, VU, 16384): (4, 4, 64, 52, 0),
    (6, VU, 65536): (13, 13, 64, 64, 0),
    # 8 channels, PCM | VU: wide, a tile of 512 frames
    (8, PCM | VU, 1): (1, 1, 64, 0, 1),
    (8, PCM | VU, 511): (1, 1, 64, 0, 1),
    (8, PCM | VU, 512): (1, 1, 64, 0, 1),
    (8, PCM | VU, 513): (2, 2, 64, 0, 0),
    (8, PCM | VU, 1024): (2, 2, 64, 0, 0),
    (8, PCM | VU, 1025): (3, 3, 64, 0, 0),
    (8, PCM | VU, 1535): (3, 3, 64, 0, 0),
    (8, PCM | VU, 1536): (3, 3, 64, 0, 0),
    (8, PCM | VU, 16384): (32, 32, 64, 0, 0),
    (8, PCM | VU, 65536): (128, 128, 64, 0, 0),
    # 8 channels, VU: rows, a tile of 4096 frames
    (8, VU, 1): (1, 1, 64, 4, 1),
    (8, VU, 4095): (1, 1, 64, 64, 1),
    (8, VU, 4096): (1, 1, 64, 64, 1),
    (8, VU, 4097): (2, 2, 64, 36, 0),
    (8, VU, 8192): (2, 2, 64, 64, 0),
    (8, VU, 8193): (3, 3, 64, 44, 0),
    (8, VU, 12287): (3, 3, 64, 64, 0),
    (8, VU, 12288): (3, 3, 64, 64, 0),
    (8, VU, 16384): (4, 4, 64, 64, 0),
    (8, VU, 65536): (16, 16, 64, 64, 0),
    # 12 channels, PCM | VU: rows, a tile of 336 frames
    (12, PCM | VU, 1): (1, 1, 64, 8, 1),
    (12, PCM | VU, 335): (1, 1, 64, 8, 1),
    (12, PCM | VU, 336): (1, 1, 64, 8, 1),
    (12, PCM | VU, 337): (2, 2, 64, 8, 0),
    (12, PCM | VU, 672): (2, 2, 64, 8, 0),
    (12, PCM | VU, 673): (3, 3, 64, 8, 0),
    (12, PCM | VU, 1007): (3, 3, 64, 8, 0),
    (12, PCM | VU, 1008): (3, 3, 64, 8, 0),
    (12, PCM | VU, 16384): (49, 49, 64, 8, 0),
    (12, PCM | VU, 65536): (196, 196, 64, 8, 0),
    # 12 channels, VU: rows, a tile of 2688 frames
    (12, VU, 1): (1, 1, 64, 4, 1),
    (12, VU, 2687): (1, 1, 64, 64, 1),
    (12, VU, 2688): (1, 1, 64, 64, 1),
    (12, VU, 2689): (2, 2, 64, 36, 0),
    (12, VU, 5376): (2, 2, 64, 64, 0),
    (12, VU, 5377): (3, 3, 64, 44, 0),
    (12, VU, 8063): (3, 3, 64, 64, 0),
    (12, VU, 8064): (3, 3, 64, 64, 0),
    (12, VU, 16384): (7, 7, 64, 56, 0),
    (12, VU, 65536): (25, 25, 64, 64, 0),
    # 16 channels, PCM | VU: rows, a tile of 256 frames
    (16, PCM | VU, 1): (1, 1, 64, 8, 1),
    (16, PCM | VU, 255): (1, 1, 64, 8, 1),
    (16, PCM | VU, 256): (1, 1, 64, 8, 1),
    (16, PCM | VU, 257): (2, 2, 64, 8, 0),
    (16, PCM | VU, 512): (2, 2, 64, 8, 0),
    (16, PCM | VU, 513): (3, 3, 64, 8, 0),
    (16, PCM | VU, 767): (3, 3, 64, 8, 0),
    (16, PCM | VU, 768): (3, 3, 64, 8, 0),
    (16, PCM | VU, 16384): (64, 64, 64, 8, 0),
    (16, PCM | VU, 65536): (256, 256, 64, 8, 0),
    # 16 channels, VU: rows, a tile of 2048 frames
    (16, VU, 1): (1, 1, 64, 4, 1),
    (16, VU, 2047): (1, 1, 64, 64, 1),
    (16, VU, 2048): (1, 1, 64, 64, 1),
    (16, VU, 2049): (2, 2, 64, 36, 0),
    (16, VU, 4096): (2, 2, 64, 64, 0),
    (16, VU, 4097): (3, 3, 64, 44, 0),
    (16, VU, 6143): (3, 3, 64, 64, 0),
    (16, VU, 6144): (3, 3, 64, 64, 0),
    (16, VU, 16384): (8, 8, 64, 64, 0),
    (16, VU, 65536): (32, 32, 64, 64, 0),
}


# the benchmark's shapes (bench.py WORKLOADS; c2 carries a channel swap, c3 runs the EQ kernel instead)
BENCH = {    # (streams, channels, frames, io, identity maps): (family, C, U, NW, grid, threads, chunks, W, rows per tile)
    (4096, 2, 65536, PCM | VU, 0): ("fast", 2, 4, 4, 65536, 256, 64, 0, 0),          # config 2
    (4096, 2, 65536, VU, 0): ("fast_ro", 2, 16, 1, 65536, 64, 16, 0, 0),              # config 2, VU only
    (8192, 1, 65536, PCM | VU, 1): ("fast", 1, 4, 4, 65536, 256, 32, 0, 0),          # configs 4 and 5
    (8192, 1, 65536, F32, 1): ("fast", 1, 4, 1, 262144, 64, 32, 0, 0),               # config 3 without sections
    (2730, 6, 16384, PCM | VU, 1): ("rows", 0, 0, 1, 68250, 64, 25, 63, 8),          # 5.1
    (2048, 6, 1 << 20, F32, 1): ("rows", 0, 0, 1, 3196928, 64, 1561, 63, 8),
    (1 << 24, 3, 65536, VU, 1): ("rows", 0, 0, 1, 117440512, 64, 7, 63, 56),         # equal read-only tiles
    (1 << 20, 16, 65536, VU, 0): ("rows", 0, 0, 1, 33554432, 64, 32, 64, 64),
    ((1 << 25) - 1, 2, 65536, PCM | VU, 1): ("fast", 2, 4, 4, 536870896, 256, 64, 0, 0),
    ((1 << 31) - 1, 1, 1, PCM | VU, 1): ("fast", 1, 4, 1, (1 << 31) - 1, 64, 1, 0, 0),
}


def plan(cm, streams, channels, frames, io, maps=1):
    return cm.plan_run(streams, channels, frames, out=io & PCM, f32=io & F32, vu=io & VU, identity_maps=maps)


@pytest.mark.parametrize("key", sorted(FORMS), ids=str)
def test_form_and_tiles_by_channels_and_outputs(cm, key):
    channels, io, maps = key
    family, c, u, nw, m, stage, chunks, w, rpt = FORMS[key]
    p = plan(cm, 4096, channels, 65536, io, maps)
    assert p["err"] == 0
    assert (p["family"], p["channels"], p["tile_u"], p["waves"], p["map"], p["stage"]) == (family, c, u, nw, m, stage)
    assert (p["chunks"], p["W"], p["rows_per_tile"]) == (chunks, w, rpt)
    assert (p["grid"], p["block"]) == (4096 * -(-chunks // nw), 64 * nw)
    assert p["keep_flag"] == 0


def test_every_form_is_covered():
    for channels in CHANNELS:
        for io in range(1, 8):
            for maps in (0, 1):
                assert (channels, io, maps) in FORMS


@pytest.mark.parametrize("key", sorted(TILES), ids=str)
def test_tiles_waves_and_flag_by_frames(cm, key):
    channels, io, frames = key
    chunks, grid, block, rpt, keep = TILES[key]
    p = plan(cm, 1, channels, frames, io)
    assert p["err"] == 0
    assert (p["chunks"], p["grid"], p["block"], p["rows_per_tile"], p["keep_flag"]) == (chunks, grid, block, rpt, keep)


@pytest.mark.parametrize("key", sorted(BENCH), ids=str)
def test_benchmark_shapes(cm, key):
    family, c, u, nw, grid, block, chunks, w, rpt = BENCH[key]
    p = plan(cm, *key)
    assert p["err"] == 0
    assert (p["family"], p["channels"], p["tile_u"], p["waves"]) == (family, c, u, nw)
    assert (p["grid"], p["block"], p["chunks"], p["W"], p["rows_per_tile"]) == (grid, block, chunks, w, rpt)
    assert p["keep_flag"] == 0


@pytest.mark.parametrize("streams, channels, frames, io", [
    (1 << 25, 2, 65536, PCM | VU),       # 64 tiles per stream: 2^31 tiles, although only 2^29 workgroups of four waves
    (1 << 31, 1, 1, PCM | VU),
    (1 << 31, 16, 1, VU),
])
def test_grid_of_2_31_tiles_is_refused(cm, streams, channels, frames, io):
    p = plan(cm, streams, channels, frames, io)
    assert p["err"] == 1                 # hipErrorInvalidValue
    assert (p["family"], p["grid"], p["keep_flag"]) == ("none", 0, 0)


@pytest.mark.parametrize("channels", CHANNELS)
def test_nothing_to_launch(cm, channels):
    # no PCM, no floats, no window; no streams; no frames
    for streams, frames, io in ((4096, 65536, 0), (1, 1, 0), (0, 65536, PCM | VU), (4096, 0, PCM | VU)):
        p = plan(cm, streams, channels, frames, io)
        assert (p["err"], p["family"], p["grid"], p["keep_flag"]) == (0, "none", 0, 0)


def test_only_single_workgroup_launches_keep_the_flag(cm):
    assert plan(cm, 1, 2, 3072, PCM | VU)["keep_flag"] == 1          # three tiles, one workgroup of four waves
    assert plan(cm, 1, 2, 4096, PCM | VU)["keep_flag"] == 1          # four tiles: still one workgroup
    assert plan(cm, 1, 2, 4097, PCM | VU)["keep_flag"] == 0          # five tiles, two workgroups
    assert plan(cm, 2, 2, 1024, PCM | VU)["keep_flag"] == 0          # two streams
    assert plan(cm, 1, 8, 512, PCM)["keep_flag"] == 1
    assert plan(cm, 1, 8, 513, PCM)["keep_flag"] == 0
