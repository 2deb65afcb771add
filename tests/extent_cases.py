"""Frames past one tile, one wave and one grid for the kernels that read the
exact accumulators (csrc/accum_kernels.hpp), and the hand-made patterns run on
them.  numpy only: tests/test_frame_extents_host.py checks the table against
the constants in the source, tests/test_gpu_frame_extents.py runs the frames.

A kernel's loop covers STEP items a pass; CROSSINGS states for every frame how
many passes each loop makes on it.  STEP's values restate the source and are
compared with it by the host test, so a constant that moves makes a frame that
no longer crosses its threshold fail there.
"""
import numpy as np

TILE = 256  # a workgroup: the columns, rows or units a list_* loop covers a pass
WAVE = 64
NOISE_BLOCKS = 2048  # kNoiseBlocks: the grid-stride kernels' largest grid
BUMP_PER_BLOCK = 4  # bump_counts_kernel: a wave per unit

# kernel -> what one pass of its loop covers
STEP = {
    "list_rows_kernel": TILE,  # columns
    "list_rows_gathered_kernel": TILE,  # columns
    "list_units_kernel": TILE,  # rows
    "list_units_kernel:wave": WAVE,  # rows one wave of its scan holds (wave_sum, before)
    "list_fill_kernel": TILE,  # units of one row
    "bump_counts_kernel": NOISE_BLOCKS * BUMP_PER_BLOCK,  # units
    "noise_kernel": NOISE_BLOCKS * TILE,  # slab pixels
    "select_over_kernel": NOISE_BLOCKS * TILE,
    "noise_active_kernel": NOISE_BLOCKS * TILE,
}

# (W, H, nsub) of every section
COLUMN_FRAMES = [(256, 3, 2), (257, 5, 2), (513, 4, 1), (770, 3, 2)]
ROW_FRAMES = [(20, 65, 2), (20, 257, 2), (7, 600, 3)]
ROW_SHARDED = (20, 600, 2)  # 2 shards of 1-row bands: 300 slab rows each
LONG_ROWS = (300, 30, 6)  # one pixel per wave: 300 units a row, 9,000 in the frame
GATHERED_FRAMES = [(513, 6, 2), (256, 4, 2), (512, 3, 1), (769, 3, 2)]
GRID_U = (1024, 513, 1)  # one device: the second grid pass is the last row
GRID_S = (1024, 1027, 1)  # band_rows 8, shards 0 and 1 of 2: 520 slab rows each
GRID_S_BAND, GRID_S_SHARDS = 8, 2
# scene, W, H, nsub, pass ends, target rho, dilate
SCHEDULES = {
    "X": ("box", 300, 300, 2, (2, 4, 8), 0.3, 1),
    "Y": ("synthetic:300", 260, 258, 2, (2, 4, 8), 0.2, 1),  # > 64 spheres: the BVH gather kernel
}
SEAM_COLUMNS = (254, 255, 256, 257, 511, 512, 513, 767, 768)


def pixels_per_wave(nsub):
    return WAVE // (nsub * nsub)


def units_per_row(W, nsub):
    return -(-W // pixels_per_wave(nsub))


def slab_rows(H, band_rows, n):
    bands = -(-H // band_rows)
    return -(-bands // n) * band_rows


def _crossings():
    """(case, kernel, the extent the kernel's loop runs over, the passes that takes)."""
    out = []
    passes = {256: 1, 257: 2, 513: 3, 770: 4}
    for W, H, nsub in COLUMN_FRAMES:
        out.append((f"columns {W}x{H}", "list_rows_kernel", W, passes[W]))
    passes = {513: 3, 256: 1, 512: 2, 769: 4}
    for W, H, nsub in GATHERED_FRAMES:
        out.append((f"gathered {W}x{H}", "list_rows_gathered_kernel", W, passes[W]))
    passes = {65: 1, 257: 2, 600: 3}
    for W, H, nsub in ROW_FRAMES:
        out.append((f"rows {W}x{H}", "list_units_kernel", H, passes[H]))
        out.append((f"rows {W}x{H}", "list_units_kernel:wave", H, {65: 2, 257: 5, 600: 10}[H]))
    W, H, nsub = ROW_SHARDED
    out.append((f"rows {W}x{H} in 2 shards", "list_units_kernel", slab_rows(H, 1, 2), 2))
    out.append((f"rows {W}x{H} in 2 shards", "list_units_kernel:wave", slab_rows(H, 1, 2), 5))
    W, H, nsub = LONG_ROWS
    out.append((f"long rows {W}x{H}", "list_fill_kernel", units_per_row(W, nsub), 2))
    out.append((f"long rows {W}x{H}", "bump_counts_kernel", H * units_per_row(W, nsub), 2))
    for k in ("noise_kernel", "select_over_kernel", "noise_active_kernel"):
        out.append(("grid U", k, GRID_U[0] * GRID_U[1], 2))
        out.append(("grid S", k, GRID_S[0] * slab_rows(GRID_S[1], GRID_S_BAND, GRID_S_SHARDS), 2))
    for name, (_, W, H, nsub, _, _, _) in SCHEDULES.items():
        out.append((f"schedule {name}", "list_rows_kernel", W, 2))
        out.append((f"schedule {name}", "list_units_kernel", H, 2))
        out.append((f"schedule {name}", "list_units_kernel:wave", H, 5))
    return out


CROSSINGS = _crossings()


# ---- patterns --------------------------------------------------------------------------------
def _uniq(out):
    seen, uniq = set(), {}
    for k, m in out.items():
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            uniq[k] = m
    return uniq


def ragged(W, H):
    """Row y has its first (5 y) % (W + 1) pixels set: unit counts differ from row to row, some rows are empty."""
    n = (5 * np.arange(H)) % (W + 1)
    return (np.arange(W)[None, :] < n[:, None]).astype(np.uint8)


def every_second(W, H):
    return ((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2).astype(np.uint8)


def column_patterns(W, H):
    """name -> bytes [H, W] for the column tiles; identical patterns are kept once."""
    z = np.zeros((H, W), np.uint8)
    out = {"none": z, "all": np.ones((H, W), np.uint8)}
    for x in SEAM_COLUMNS + (W - 1,):
        if x < W:
            m = z.copy()
            m[H // 2, x] = 1
            out[f"x{x}"] = m
    row = z.copy()
    row[min(1, H - 1)] = 1
    out["full_row"] = row
    if W > 256:
        col = z.copy()
        col[:, 256] = 7  # any non-zero byte
        out["column256"] = col
    out["every_second"] = every_second(W, H)
    corners = z.copy()
    corners[0, 0] = corners[0, W - 1] = corners[H - 1, 0] = corners[H - 1, W - 1] = 1
    out["corners"] = corners
    return _uniq(out)


def row_patterns(W, H):
    """name -> bytes [H, W] for the row tiles and waves."""
    z = np.zeros((H, W), np.uint8)
    rows = z.copy()
    for y in (63, 64, 255, 256, H - 1):
        if y < H:
            rows[y] = 1
    alt = np.repeat((np.arange(H) % 2).astype(np.uint8)[:, None], W, axis=1)
    return _uniq({"ragged": ragged(W, H), "rows": rows, "alternate_rows": alt, "all": np.ones((H, W), np.uint8),
                  "none": z})


def long_row_masks(W, H):
    return {"all": np.ones((H, W), np.uint8), "every_second": every_second(W, H), "ragged": ragged(W, H)}


def grid_count_masks(W, valid_rows):
    """The two masks [valid_rows, W] that give the grid-stride frames counts of 0, 2 and 4 (2 samples
    under each): 0 in columns 1000..1023 and in the last valid row, 4 where (x // 64 + y) is even; y the
    image row of each valid slab row."""
    y = np.asarray(valid_rows)
    x = np.arange(W)
    first = np.ones((len(y), W), dtype=bool)
    first[:, 1000:1024] = False
    first[-1] = False
    second = first & (((x[None, :] // 64 + y[:, None]) % 2) == 0)
    return first.astype(np.uint8), second.astype(np.uint8)
