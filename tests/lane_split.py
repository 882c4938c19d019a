"""A plain mirror of how the two Snappy lane-decoder launches deal records to lanes.

The tests use it only to prove that a file reaches the code they name (records per lane, which
records share a lane, which lane comes up short); never to compute expected bytes.

The three kernel constants it copies:
"""
GRID = 512            # RIO_SNAPPY_GRID's default (kSnappyGrid), csrc/rio_device.h
WAVES_PER_GROUP = 4   # kSnappyBlock / 64, csrc/rio_device.h
CHUNKS_PER_WAVE = 8   # kChunksPerWave, csrc/rio_snappy.hip

WAVES = GRID * WAVES_PER_GROUP


def pipe_split(n):
    """k_snappy_pipe (one file of n records): (rpc, [(r0, r1) per lane]), the lanes in chunk order,
    64 to a wave. Which wave of the grid takes a chunk past the first WAVES is decided at run time;
    the chunk's record ranges are not."""
    rpc = n // (CHUNKS_PER_WAVE * 64 * WAVES) if n >= CHUNKS_PER_WAVE * 64 * WAVES else 1
    per = 64 * rpc
    nchunks = (n + per - 1) // per
    lanes = []
    for chunk in range(nchunks):
        for lane in range(64):
            r0 = min(chunk * per + lane * rpc, n)
            lanes.append((r0, min(r0 + rpc, n)))
    return rpc, lanes


def batch_split(counts):
    """k_snappy_pipe_batch over one launch group: `counts` are the record counts of the group's
    lane-decoder files (Snappy files that are not all-literal, wide or handed to the wave-per-record
    decoder; other files take no part). Returns (rpl, [[(r0, r1) per lane] per file])."""
    total = sum(counts)
    if total == 0:
        return 0, [[] for _ in counts]
    rpl = (total + 64 * WAVES - 1) // (64 * WAVES)
    while True:
        need = sum((n + 64 * rpl - 1) // (64 * rpl) for n in counts)
        if need <= WAVES:
            break
        rpl += 1
    per_wave = 64 * rpl
    files = []
    for n in counts:
        wf = (n + per_wave - 1) // per_wave
        lanes = []
        for t in range(wf * 64):
            r0 = min(t * rpl, n)
            lanes.append((r0, min(r0 + rpl, n)))
        files.append(lanes)
    return rpl, files
