"""Tile-range partitioning of a long stereo stream: chunks for one GPU, shards for N GPUs.

The reference processes a spectrogram as independent, non-overlapping T-frame tiles with no cross-tile state
(Executable/main.c:455-495); its own multi-thread mode hands contiguous tile ranges to threads (main.c:545-575).
Here the same ranges go to GPUs (one process per GPU) and, inside a GPU, to batches of at most `max_tiles` tiles.
A range [j0, j1) needs the PCM samples [j0*T*1024, j1*T*1024 + 3072) and produces the overlap-add contribution of
its own frames, which covers output samples [j0*T*1024, j1*T*1024 + 3072): consecutive ranges overlap by 3072
samples and are simply ADDED when stitched.  No data-path collective exists; weights are broadcast once.
"""
from collections import namedtuple

HOP, FFT = 1024, 4096

Chunk = namedtuple("Chunk", "tile0 tile1 sample0 nsamples frames rows out_offset")


def stft_rows(n):
    return (n + HOP - 1) // HOP                                   # stftFix.c:367


def stft_frames(n):
    return 0 if n < FFT else (n - FFT + HOP // 4) // HOP + 1      # stftFix.c:378 + the tail frame


def rank_tiles(ntiles, rank, world):
    """Contiguous tile range of one rank (GPU g gets tiles [g*ceil(N/G), ...))."""
    per = (ntiles + world - 1) // world
    return min(rank * per, ntiles), min((rank + 1) * per, ntiles)


def plan(n, T, max_tiles, rank=0, world=1):
    """Chunks (<= max_tiles tiles each) this rank has to run for an n-sample stream."""
    rows, frames = stft_rows(n), stft_frames(n)
    ntiles = (rows + T - 1) // T
    t0, t1 = rank_tiles(ntiles, rank, world)
    out = []
    j = t0
    while j < t1:
        j1 = min(j + max_tiles, t1)
        row0, row1 = j * T, min(j1 * T, rows)
        s0 = row0 * HOP
        ns = min(n, row1 * HOP + (FFT - HOP)) - s0
        out.append(Chunk(j, j1, s0, ns, max(0, min(frames - row0, row1 - row0)), row1 - row0, s0))
        j = j1
    return out


Span = namedtuple("Span", "tile0 tile1 sample0 nsamples frames rows out_offset")


def rank_span(n, T, rank=0, world=1):
    """The contiguous tile range of one rank as ONE span (what srtSeparateHostStream chunks natively): tiles
    [tile0, tile1), PCM samples [sample0, sample0 + nsamples) (3072-sample halo included), `frames` transformed
    frames, `rows` rows, and the offset of its overlap-add contribution in the full output."""
    rows, frames = stft_rows(n), stft_frames(n)
    ntiles = (rows + T - 1) // T
    t0, t1 = rank_tiles(ntiles, rank, world)
    row0, row1 = t0 * T, min(t1 * T, rows)
    s0 = row0 * HOP
    ns = max(0, min(n, row1 * HOP + (FFT - HOP)) - s0)
    return Span(t0, t1, s0, ns, max(0, min(frames - row0, row1 - row0)), max(0, row1 - row0), s0)


BatchGroup = namedtuple("BatchGroup", "tracks tile0 ntiles")


def pack_tracks(ns, T, max_tiles, overlap=0):
    """Greedy grouping, in order, of independent tracks of ns[k] samples into srtSeparateBatch calls of at most max_tiles packed
    tiles: a call takes tracks until the next one would not fit.  Track k takes ceil(stft_rows(ns[k]) / T) tiles, packed from
    tile0; with overlap = O > 0 (srtSeparateBatchOverlap, srtBatchPlanOverlap) it takes overlap_tiles(stft_rows(ns[k]), T, O).
    Returns [BatchGroup(tracks = indices into ns, tile0 = each track's first tile in its call, ntiles = the call's total)]."""
    groups, cur, tile0, used = [], [], [], 0
    for k, n in enumerate(ns):
        if n < FFT:
            raise ValueError("track %d: %d samples, at least %d needed" % (k, n, FFT))
        nt = overlap_tiles(stft_rows(n), T, overlap)
        if nt > max_tiles:
            raise ValueError("track %d alone takes %d tiles, more than max_tiles = %d: separate it with the chunked paths" % (k, nt, max_tiles))
        if used + nt > max_tiles:
            groups.append(BatchGroup(cur, tile0, used))
            cur, tile0, used = [], [], 0
        cur.append(k)
        tile0.append(used)
        used += nt
    if cur:
        groups.append(BatchGroup(cur, tile0, used))
    return groups


def overlap_tiles(rows, T, O):
    """srtOverlapTiles: network tiles of a signal of `rows` spectrum rows when consecutive tiles share O rows (0 <= O <= T/2).
    Stride S = T - O, tile j covers rows [jS, jS + T): one tile up to T rows, else ceil((rows - O) / S) - every tile then owns at least one row
    that no earlier tile covers, and the tiles cover all rows.  O = 0 is ceil(rows / T)."""
    if T < 1 or O < 0 or O > T // 2:
        raise ValueError("overlap_tiles: need T >= 1 and 0 <= O <= T / 2 (T = %d, O = %d)" % (T, O))
    if rows <= 0:
        return 0
    S = T - O
    return 1 if rows <= T else (rows - O + S - 1) // S


def host_overlap_pieces(rows, T, O, max_tiles):
    """srtHostOverlapPieces: the pieces srtSeparateHostStreamOverlap walks a stream of `rows` spectrum rows in, a list of dicts tile0 / tiles /
    row0 / own_rows / stft_rows.  With S = T - O and N = overlap_tiles(rows, T, O), piece p holds tiles [p max_tiles, min((p + 1) max_tiles, N)), owns the rows
    whose primary tile is one of them - max_tiles * S from row0 = tile0 * S, the last piece up to `rows` - and analyses the rows its tiles cover,
    (tiles - 1) S + T from row0 (the last piece: what is left): O of them are the next piece's.  O = 0 is the chunking of separate_host_stream."""
    if max_tiles < 1:
        raise ValueError("host_overlap_pieces: need max_tiles >= 1 (max_tiles = %d)" % max_tiles)
    N, S = overlap_tiles(rows, T, O), T - O
    pieces = []
    for tile0 in range(0, N, max_tiles):
        tiles = min(max_tiles, N - tile0)
        row0 = tile0 * S
        own = rows - row0 if tile0 + tiles == N else tiles * S
        pieces.append(dict(tile0=tile0, tiles=tiles, row0=row0, own_rows=own, stft_rows=min(rows - row0, (tiles - 1) * S + T)))
    return pieces


def rs_geometry(fs_in, fs_out, table_len=22438, index_inc=491):
    """The converter's geometry for a rate pair (csrc/srt_resample.hip:srt_rs_geometry; defaults: the built-in filter's layout): dict P, Q (the rates over their
    gcd), LO (a frame at input position i + frac takes input frames i - LO .. i + LO + 1) and T4 (the window's taps, padded to a multiple of 4 with zero weights)."""
    from math import gcd
    g = gcd(fs_in, fs_out)
    inc = int(round(index_inc * min(fs_out / fs_in, 1.0) * 4096.0))      # rint: halves to even, as round()
    LO = ((table_len - 2) << 12) // inc
    return dict(P=fs_in // g, Q=fs_out // g, LO=LO, T4=(2 * LO + 2 + 3) // 4 * 4)


def rs_computable(geom, n_in):
    """srtResampleComputable: output frames whose last weighted tap, floor(j P / Q) + LO + 1, lies before input frame n_in"""
    a = n_in - (geom["LO"] + 1)
    return 0 if a <= 0 else -(-a * geom["Q"] // geom["P"])


def resample_length(n, fs_in, fs_out):
    """srtResampleLength: ceil(n * (fs_out / fs_in)) in doubles, as the reference allocates"""
    from math import ceil
    return int(ceil(float(n) * (fs_out / float(fs_in))))


def host_rate_length(n, in_rate, out_rate):
    """srtHostRateLength: frames per output plane of srtSeparateHostStreamRate for n frames at in_rate"""
    n44 = n if in_rate == 44100 else resample_length(n, in_rate, 44100)
    len44 = stft_rows(n44) * 1024 + 3072
    return len44 if out_rate == 44100 else resample_length(len44, 44100, out_rate)


def host_rate_pieces(n, in_rate, out_rate, T, O, max_tiles):
    """srtHostRatePieces: the pieces srtSeparateHostStreamRate walks n frames at in_rate in, a list of dicts.  Piece c of host_overlap_pieces over
    the 44.1 kHz stream analyses samples [s0, s0 + ns) and finalises [fin0, fin1) of every output plane (fin1 = s0 + own_rows * 1024, the last piece to the end).
    With (P, Q, LO, T4) of in_rate -> 44100 it uploads source frames [src0, src0 + src_len) = [max(0, floor(s0 P / Q) - LO), min(n, floor((s0 + ns - 1) P / Q) -
    LO + T4)); with the geometry of 44100 -> out_rate it emits output frames [out0, out1), out = min(len_out, rs_computable(fin)), the last piece to len_out.  A
    side at 44100 has no converter: src = (s0, ns), out = fin."""
    for r in (in_rate, out_rate):
        if r < 8000 or r > 384000:
            raise ValueError("host_rate_pieces: sample rates must lie in 8000..384000 Hz (%d)" % r)
    n44 = n if in_rate == 44100 else resample_length(n, in_rate, 44100)
    if n44 < 4096:
        raise ValueError("host_rate_pieces: need at least 4096 samples at 44.1 kHz (%d)" % n44)
    rows = stft_rows(n44)
    len44 = rows * 1024 + 3072
    len_out = host_rate_length(n, in_rate, out_rate)
    gi = rs_geometry(in_rate, 44100) if in_rate != 44100 else None
    go = rs_geometry(44100, out_rate) if out_rate != 44100 else None
    plan = host_overlap_pieces(rows, T, O, max_tiles)
    pieces = []
    for c, pc in enumerate(plan):
        last = c + 1 == len(plan)
        s0 = pc["row0"] * 1024
        send = min((pc["row0"] + pc["stft_rows"]) * 1024 + 3072, n44)
        ns = max(send - s0, 0)
        src0, src_len = s0, ns
        if gi:
            lo = hi = 0
            if ns:
                lo = max(s0 * gi["P"] // gi["Q"] - gi["LO"], 0)
                hi = max(min((send - 1) * gi["P"] // gi["Q"] - gi["LO"] + gi["T4"], n), lo)
            src0, src_len = lo, hi - lo
        fin0, fin1 = s0, len44 if last else s0 + pc["own_rows"] * 1024
        out0, out1 = fin0, fin1
        if go:
            out0 = min(rs_computable(go, fin0), len_out)
            out1 = len_out if last else min(rs_computable(go, fin1), len_out)
        pieces.append(dict(src0=src0, src_len=src_len, s0=s0, ns=ns, fin0=fin0, fin1=fin1, out0=out0, out1=out1))
    return pieces


def _refuse_overlap(engine):
    """The chunked and ranked paths cut a stream at back-to-back tile boundaries; with overlapped tiles the blend would have to cross those seams."""
    if getattr(engine, "overlap", 0):
        raise ValueError("overlapped tiles (set_overlap > 0) are not available on the chunked / ranked paths: the mask blend would have to cross "
                         "the chunk seams; set_overlap(0), or separate() a signal that fits the engine")


def _refuse_wiener(engine, world):
    """The Wiener filter's statistics span the whole signal: ranks would each filter their range with its own covariance."""
    if world > 1 and getattr(engine, "wiener", 0):
        raise ValueError("the Wiener filter's statistics span the whole signal: a rank's share (world = %d) would get its own covariance; "
                         "set_wiener(0) or run one rank" % world)


def separate_host_range(engine, L, R, rank=0, world=1, out=None, pinned=False):
    """This rank's share of a HOST-resident stream (numpy / pinned arrays of the whole stream, or anything sliceable):
    one srtSeparateHostStream call over its tile range — chunks of engine.max_tiles tiles, H2D / compute / D2H overlapped
    on three HIP streams, chunk overlaps carried on the device.  Returns (span, stems [S,2,rows*1024+3072]) or
    (span, None) when the rank has no tiles.  The reference's counterpart is one tile-range worker of processMT
    (Executable/main.c:544-673); there is no exchange with other ranks."""
    _refuse_wiener(engine, world)
    _refuse_overlap(engine)
    sp = rank_span(len(L), engine.T, rank, world)
    if sp.rows == 0:
        return sp, None
    o = engine.separate_host_stream(L[sp.sample0:sp.sample0 + sp.nsamples], R[sp.sample0:sp.sample0 + sp.nsamples],
                                    frames=sp.frames, rows=sp.rows, out=out, pinned=pinned)
    return sp, o


def total_output_length(n):
    return stft_rows(n) * HOP + (FFT - HOP)                       # stftFix.c:500


def separate_stream(engine, L, R, rank=0, world=1):
    """Run this rank's chunks.  `engine` needs .T, .max_tiles and .separate_ex(L, R, frames, rows) -> [S,2,rows*1024+3072]
    (spleeterrt_amd.Engine on a GPU; tests substitute a CPU stand-in).  Returns [(out_offset, array)]."""
    _refuse_wiener(engine, world)
    _refuse_overlap(engine)
    parts = []
    for c in plan(len(L), engine.T, engine.max_tiles, rank, world):
        o = engine.separate_ex(L[c.sample0:c.sample0 + c.nsamples], R[c.sample0:c.sample0 + c.nsamples], c.frames, c.rows)
        parts.append((c.out_offset, o))
    return parts


def stitch(parts, n, nstems):
    """Add the (offset, [S,2,len]) contributions of all chunks / ranks into the full-length output (host side)."""
    import numpy as np
    out = np.zeros((nstems, 2, total_output_length(n)), np.float32)
    for off, o in sorted(parts, key=lambda p: p[0]):
        o = o.detach().cpu().numpy() if hasattr(o, "detach") else np.asarray(o)
        out[:, :, off:off + o.shape[2]] += o
    return out


def init_distributed(device=None):
    """One process per GPU.  Under a torch.distributed launcher (RANK / WORLD_SIZE / MASTER_ADDR in the environment) join the
    process group - `nccl` (= RCCL on ROCm) when `device` is a GPU, gloo otherwise - at ANY world size, 1 included: a world of one
    still loads RCCL and runs the weight broadcast, so the N > 1 code path is the one that always runs.  Returns (rank, world, on)."""
    import os
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ and "MASTER_ADDR" in os.environ
    if (world > 1 or launched) and not dist.is_initialized():
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC
        if device is not None and str(device).startswith("cuda"):
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group("gloo")
    return rank, world, dist.is_initialized()


def broadcast_weights(coeffs, device=None, src=0):
    """The one collective of the path: rank `src` holds the blobs (list of float32 arrays/tensors, one per stem),
    every rank gets them (RCCL over xGMI when the process group is `nccl`, gloo on CPU)."""
    import torch
    import torch.distributed as dist
    n = 9822725
    k = [len(coeffs) if coeffs is not None else 0]
    if dist.is_initialized():
        dist.broadcast_object_list(k, src)
    out = []
    for s in range(k[0]):
        if coeffs is not None:
            t = torch.as_tensor(coeffs[s], dtype=torch.float32).reshape(-1).to(device or "cpu")
        else:
            t = torch.empty(n, dtype=torch.float32, device=device or "cpu")
        if dist.is_initialized():
            dist.broadcast(t, src)
        out.append(t)
    return out
