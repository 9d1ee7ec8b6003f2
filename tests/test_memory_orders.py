"""Every memory order vtmc_extract_grid accepts ("any positive strides", include/vtmc.h), and the C# host's own array -- a
float[W+2, E+2, H+2], z fastest -- at the largest size the reference takes, 1026^3 samples.

In z-fastest order the large stride is sx = 1026^2: a block's origin lies more than 2^31 bytes from the grid base from bx = 64 on,
and the last x slabs more than 2^32 bytes.  A 32-bit truncation of a base or slab offset would corrupt the far x face only, which
neither a 64^3 grid nor a count-only check can see; so the full-size tests compare records, block by block, on the far x face.

Bars: exact mode (emit_fast_math=0) -- offsets, cases, block ids and every float equal to the oracle's bit for bit (a zero may differ
in sign, as in test_gpu_parity.py's exact-mode test), NaN patterns equal; fast mode (the shipped default) -- offsets and block ids
equal, floats within 2e-6 of the oracle.  Between two layouts of the same field on the device the bar is byte identity.

The mid-size tests come first, the 1026^3 ones last (unranked GPU tests run in file order)."""
import numpy as np
import pytest

import fields
from extract_checks import check_against_oracle, device_view_i32, smooth_field
from surface_twin import _cast, _long_rays

FAST_ATOL = 2e-6
ROW = 19   # int32 words of one 76-byte record: 18 floats and the block id

# memory order, slowest axis first: "zyx" is x fastest (the build's native layout), "xyz" the C# float[,,]
ORDERS = ("zyx", "yzx", "zxy", "xzy", "yxz", "xyz")

# cells per axis: nz covers the z-lane streaming classify's full and partial 64-lane segments, nx / ny stay small
SHAPES = [(8, 8, 32), (16, 24, 40), (48, 8, 64), (8, 24, 72), (16, 8, 136), (48, 24, 200),
          (48, 24, 32), (16, 8, 200), (8, 24, 64), (48, 8, 40), (8, 8, 136), (16, 24, 72)]

N, DIM = 1024, 1026
NB = N // 8
T_1026 = 42487270   # perlin3d at 1026^3 (test_gpu_parity.py::test_max_size_single_grid_equals_chunked)


# ---- layouts -------------------------------------------------------------------------------------------------------------------

def pitches(dims, order, pad=(0, 0)):
    """Memory dims (slowest first), the pitches of the slowest and the middle axis, and the elements the layout spans, for dims
    samples per axis (x, y, z) in memory order `order`; pad = extra elements in the middle and in the slowest pitch."""
    m = [dims["xyz".index(a)] for a in order]
    p1 = m[2] + pad[0]
    p0 = p1 * m[1] + pad[1]
    return m, p0, p1, p0 * m[0]


def strided_view(buf, offset, dims, order, pad=(0, 0)):
    """A view of buf[offset:] indexed [x, y, z], laid out as pitches() says."""
    m, p0, p1, span = pitches(dims, order, pad)
    assert offset + span <= buf.size
    mem = np.lib.stride_tricks.as_strided(buf[offset:], shape=m, strides=(4 * p0, 4 * p1, 4))
    return mem.transpose(np.argsort(["xyz".index(a) for a in order]))


def laid_out(g, order, pad=(0, 0), seed=0):
    """g (indexed [x, y, z]) copied into memory order `order`; the padding holds random samples of both signs."""
    span = pitches(g.shape, order, pad)[3]
    buf = (np.random.default_rng(seed).standard_normal(span) * 3).astype(np.float32)
    view = strided_view(buf, 0, g.shape, order, pad)
    view[...] = g
    assert np.array_equal(view, g)
    return view


def layouts(g, seed):
    """(label, grid) for all six orders, tight (a transposed C-contiguous array) and padded (both outer pitches padded)."""
    out = []
    for i, order in enumerate(ORDERS):
        out.append((order + "/tight", laid_out(g, order)))
        out.append((order + "/padded", laid_out(g, order, pad=(3 + i, 5 + 2 * i), seed=seed + i)))
    return out


def host_span(grid):
    """Elements vtmc_extract_grid's host paths see as the grid's extent (vtmc_api.hip: upload_grid)."""
    sx, sy, sz = (s // 4 for s in grid.strides)
    nx, ny, nz = (d - 2 for d in grid.shape)
    return (nx + 1) * sx + (ny + 1) * sy + (nz + 1) * sz + 1


# ---- comparisons ---------------------------------------------------------------------------------------------------------------

def float_bits(a):
    """uint32 words of a float array with -0 folded onto +0 (the exact mode's one allowed difference)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return u


def assert_soup(got, want, exact, what=""):
    """Records against the oracle: block ids equal; exact: float bits equal (up to the sign of zero), else within FAST_ATOL."""
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got["block"], want["block"]), what
    for f in ("p0", "p1", "p2", "n0", "n1", "n2"):
        g, w = got[f], want[f]
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, "NaN pattern", f)
        if exact:
            assert np.array_equal(float_bits(g), float_bits(w)), (what, "bits", f)
        else:
            d = np.abs(np.where(nan, 0, g) - np.where(nan, 0, w)).max(initial=0.0)
            assert d <= FAST_ATOL, (what, f, float(d))


def rows_of(buf, width, offs, ids):
    """Rows of the listed blocks out of a whole-grid result, in list order: buf holds `width` words per row, offs the per-block row
    offsets in canonical block order, ids the canonical block ids (repeats allowed).  torch tensors on any device.
    Returns (rows [n, width], rows per listed block)."""
    import torch
    ids = torch.as_tensor(np.asarray(ids, np.int64), device=offs.device)
    start = offs[ids].long()
    cnt = offs[ids + 1].long() - start
    first = torch.cumsum(cnt, 0) - cnt
    which = torch.repeat_interleave(torch.arange(len(ids), device=offs.device), cnt)
    pos = start[which] + torch.arange(int(cnt.sum()), device=offs.device) - first[which]
    return buf.view(-1, width)[pos], cnt


def float_gap(a, b, chunk=1 << 22):
    """(block ids equal, NaN patterns equal, max |a - b| over the floats) of two [n, 19] int32 record arrays, chunk by chunk."""
    import torch
    assert a.shape == b.shape
    ids_ok, nan_ok, worst = True, True, 0.0
    for i in range(0, a.shape[0], chunk):
        x, y = a[i:i + chunk], b[i:i + chunk]
        ids_ok &= bool(torch.equal(x[:, 18], y[:, 18]))
        fx, fy = x.view(torch.float32)[:, :18], y.view(torch.float32)[:, :18]
        nan_ok &= bool(torch.equal(torch.isnan(fx), torch.isnan(fy)))
        worst = max(worst, float(torch.nan_to_num(fx - fy, nan=0.0).abs().max()))
    return ids_ok, nan_ok, worst


def ids_of(blocks):
    """Canonical block ids bx + nb (by + nb bz) of a full-size grid."""
    blocks = np.asarray(blocks, np.int64)
    return blocks[:, 0] + NB * (blocks[:, 1] + NB * blocks[:, 2])


def far_face_blocks(seed=5):
    """The blocks the full-size tests check against the oracle: every block with bx = 127 (their tiles reach past 2^32 bytes in
    z-fastest order), every block with bx in {63, 64} (the origins straddle 2^31 bytes), the 8 corners and 2000 seeded random ones."""
    a = np.arange(NB)
    by, bz = (v.ravel() for v in np.meshgrid(a, a, indexing="ij"))
    parts = [np.stack([np.full_like(by, bx), by, bz], 1) for bx in (NB - 1, NB // 2 - 1, NB // 2)]
    parts.append(np.array([[x, y, z] for z in (0, NB - 1) for y in (0, NB - 1) for x in (0, NB - 1)]))
    parts.append(np.random.default_rng(seed).integers(0, NB, size=(2000, 3)))
    return np.concatenate(parts).astype(np.int32)


def check_blocks_against_oracle(rows, cnt, want, want_offs, ids, what):
    """Records gathered per listed block (rows_of) against the oracle's extract over the same list, exact bar."""
    assert np.array_equal(cnt.cpu().numpy(), np.diff(want_offs)), what
    got = rows.cpu().numpy().view(oracle_tri_dtype()).reshape(-1).copy()
    assert np.array_equal(got["block"], ids[want["block"]]), what      # the device writes canonical ids, the oracle list positions
    got["block"] = want["block"]
    assert_soup(got, want, exact=True, what=what)


def oracle_tri_dtype():
    import oracle
    return oracle.TRI_DTYPE


# ---- the comparisons bite (no GPU) ---------------------------------------------------------------------------------------------

def test_record_comparisons_report_one_flipped_bit_and_one_dropped_triangle():
    """The comparisons the full-size tests use, on a synthetic whole-grid result: one flipped float bit in a far-face block and one
    triangle dropped from an offsets copy are both reported; the per-block gather returns exactly each block's records."""
    import torch
    rng = np.random.default_rng(3)
    nb = 4
    counts = rng.integers(0, 5, nb ** 3)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    T = int(offs[-1])
    rec = np.zeros((T, ROW), np.int32)
    rec[:, :18] = rng.standard_normal((T, 18)).astype(np.float32).view(np.int32)
    rec[:, 18] = np.repeat(np.arange(nb ** 3), counts)
    tris = torch.from_numpy(rec.reshape(-1))
    far = [b for b in range(nb ** 3) if b % nb == nb - 1 and counts[b] > 0]
    ids = np.array(far + [0, far[0], 5], np.int64)
    rows, cnt = rows_of(tris, ROW, offs, ids)
    assert np.array_equal(cnt.numpy(), counts[ids])
    assert np.array_equal(rows.numpy(), np.concatenate([rec[offs[b]:offs[b + 1]] for b in ids]))
    # one bit of one float of a block on the far x face
    b = far[-1]
    bad = tris.clone()
    bad[int(offs[b]) * ROW + 4] ^= 1
    assert torch.equal(tris, tris.clone()) and not torch.equal(bad, tris)
    ids_ok, nan_ok, worst = float_gap(bad.view(-1, ROW), tris.view(-1, ROW))
    assert ids_ok and nan_ok and worst > 0.0
    r_bad, _ = rows_of(bad, ROW, offs, [b])
    got = r_bad.numpy().view(oracle_tri_dtype()).reshape(-1).copy()
    want = rows_of(tris, ROW, offs, [b])[0].numpy().view(oracle_tri_dtype()).reshape(-1).copy()
    want["block"] = got["block"] = 0
    with pytest.raises(AssertionError):
        assert_soup(got, want, exact=True)
    assert_soup(got, want, exact=False)      # one ulp: inside the fast-mode bar, outside the exact one
    # one triangle dropped from block b
    short = offs.clone()
    short[b + 1:] -= 1
    assert not torch.equal(short, offs)
    _, c_short = rows_of(tris, ROW, short, [b])
    assert int(c_short[0]) == counts[b] - 1


# ---- 1. every memory order, mid-size -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ex():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import volumetricterrain_amd as vt
    e = vt.Extractor(0)
    yield e
    e.close()


def make_field(kind, shape, seed):
    if kind == "random":
        return fields.random_field(shape, seed=seed)
    return smooth_field(np.random.default_rng(seed), shape, "x")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_every_memory_order_matches_the_oracle(ex, oracle_mod, shape, kind):
    """All six axis orders, tight and padded, through vtmc_extract_grid: soup in exact mode (with the cases of the WANT_CASES block
    path) and in fast mode, the indexed output, and dirty lists in arbitrary order with repeats (one short enough for the host tile
    gather, one long enough for the upload and device block list)."""
    seed = 100 * shape[0] + 10 * shape[1] + shape[2] + (7 if kind == "smooth" else 0)
    g = make_field(kind, shape, seed)
    want, want_offs, want_cases = oracle_mod.extract_grid(g, want_cases=True, threads=8)
    grids = layouts(g, seed)
    try:
        ex.set_tuning(emit_fast_math=0)
        for label, gl in grids:
            assert ex.extract_grid(gl) == len(want), label
            got, offs = ex.read_triangles()
            assert np.array_equal(offs, want_offs), label
            assert np.array_equal(ex.read_cases(), want_cases), label
            assert_soup(got, want, exact=True, what=label)
    finally:
        ex.set_tuning(emit_fast_math=1)
    for label, gl in grids:
        assert ex.extract_grid(gl) == len(want), label
        got, offs = ex.read_triangles()
        assert np.array_equal(offs, want_offs), label
        assert_soup(got, want, exact=False, what=label)
    try:
        ex.set_output_mode(True)
        for label, gl in grids:
            check_against_oracle(ex, oracle_mod, gl)
    finally:
        ex.set_output_mode(False)
    allb = oracle_mod.all_blocks(*shape)
    rng = np.random.default_rng(seed)
    for label, gl in grids:
        n_gather = (host_span(gl) - 1) // 2000            # vtmc_extract_grid gathers tiles on the host below span / 2000 blocks
        lengths = [3 * len(allb) + 1] + ([int(rng.integers(1, n_gather + 1))] if n_gather >= 1 else [])
        for n in lengths:
            blocks = allb[rng.integers(0, len(allb), size=n)]
            w, w_offs, _ = oracle_mod.extract_grid(g, blocks, threads=4)
            assert ex.extract_grid(gl, blocks) == len(w), (label, n)
            got, offs = ex.read_triangles()
            assert np.array_equal(offs, w_offs), (label, n)
            assert_soup(got, w, exact=False, what=(label, n))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["xyz", "yxz", "zxy", "xzy"])   # z fastest (x or y slowest), y fastest (z or x slowest)
@pytest.mark.parametrize("shape,n_vol", [((16, 24, 72), 3), ((48, 8, 136), 2), ((8, 16, 40), 3)], ids=["16x24x72", "48x8x136", "8x16x40"])
def test_padded_volume_batches_in_other_orders_on_the_device(ex, oracle_mod, shape, n_vol, order):
    """vtmc_extract_volumes_device on batches of z-fastest and y-fastest volumes with padded pitches and a padded volume stride:
    the counterpart of test_random_shapes.py's x-fastest batches.  Exact mode bit for bit, fast mode within FAST_ATOL."""
    import torch
    rng = np.random.default_rng(10 * shape[2] + ORDERS.index(order))
    dims = tuple(d + 2 for d in shape)
    pad = (int(rng.integers(1, 7)), int(rng.integers(1, 40)))
    vs = pitches(dims, order, pad)[3] + int(rng.integers(1, 33))
    host = (rng.standard_normal(n_vol * vs) * 3).astype(np.float32)   # the padding holds samples of both signs
    bpv = (shape[0] // 8) * (shape[1] // 8) * (shape[2] // 8)
    want = []
    for v in range(n_vol):
        g = smooth_field(rng, shape, "x") if v % 2 else fields.random_field(shape, seed=v + shape[2])
        view = strided_view(host, v * vs, dims, order, pad)
        view[...] = g
        t, _, _ = oracle_mod.extract_grid(g, threads=4)
        t = t.copy()
        t["block"] += v * bpv
        want.append(t)
    want = np.concatenate(want)
    strides = tuple(s // 4 for s in view.strides)
    assert strides[2 if order[-1] == "z" else 1] == 1
    d = torch.from_numpy(host).cuda()
    try:
        ex.set_tuning(emit_fast_math=0)
        assert ex.extract_volumes_device(d.data_ptr(), shape, strides, n_vol, vs) == len(want)
        got, _ = ex.read_triangles()
        assert_soup(got, want, exact=True, what=order)
    finally:
        ex.set_tuning(emit_fast_math=1)
    assert ex.extract_volumes_device(d.data_ptr(), shape, strides, n_vol, vs) == len(want)
    got, _ = ex.read_triangles()
    assert_soup(got, want, exact=False, what=order)
    _, _, vc_ptr = ex.device_results()
    vc = ex.copy_u32(vc_ptr, 2 * n_vol).reshape(n_vol, 2)
    assert np.array_equal(vc[:, 1], np.bincount(want["block"] // bpv, minlength=n_vol))


# ---- 2. the C# array at full size, on the device -------------------------------------------------------------------------------

def fill_1026(ex, order):
    """A 1026^3 perlin3d grid filled by the device sampler: order 'x' = strides (1, dim, dim^2), 'z' = (dim^2, dim, 1)."""
    import torch
    import volumetricterrain_amd as vt
    strides = (1, DIM, DIM * DIM) if order == "x" else (DIM * DIM, DIM, 1)
    g = torch.empty(DIM ** 3, dtype=torch.float32, device="cuda")
    ex.density_fill_device(vt.density_params("perlin3d", N), [[0, 0, 0]], (DIM, DIM, DIM), strides, 0, g.data_ptr())
    return g, strides


def soup_on_device(ex, grid, strides):
    """(T, records [T, 19] int32, offsets [B+1] int32): zero-copy views of the library's buffers (valid until its next extract)."""
    T = ex.extract_volumes_device(grid.data_ptr(), (N, N, N), strides, 1, 0)
    tri_ptr, off_ptr, _ = ex.device_results()
    return T, device_view_i32(tri_ptr, T * ROW).view(-1, ROW), device_view_i32(off_ptr, NB ** 3 + 1)


def host_copy_z(gz):
    """The z-fastest device grid as a host array indexed [x, y, z] (a C# float[,,])."""
    return gz.view(DIM, DIM, DIM).cpu().numpy()


def free_gpu():
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_csharp_array_1026_soup_and_rays_on_the_device(oracle_mod):
    """One perlin3d field filled in both layouts at 1026^3: the fills are bit-identical; the exact-mode soups of the two layouts
    have T = 42 487 270, equal offsets and byte-identical records; the far x face, the 2^31-byte boundary, the corners and random
    blocks of the z-fastest grid equal the oracle record by record; fast mode keeps offsets and ids and stays within 2e-6 of
    exact mode, and its records are byte-identical between the layouts; 256 long diagonal rays hit the same points in both layouts."""
    import torch
    import volumetricterrain_amd as vt
    ex = vt.Extractor(0)
    try:
        gx, sx = fill_1026(ex, "x")
        gz, sz = fill_1026(ex, "z")
        vx, vz = gx.view(DIM, DIM, DIM).permute(2, 1, 0), gz.view(DIM, DIM, DIM)   # both [x, y, z]
        for x0 in range(0, DIM, 128):
            assert torch.equal(vx[x0:x0 + 128].view(torch.int32), vz[x0:x0 + 128].view(torch.int32)), "fills differ at x >= %d" % x0
        del vx, vz

        # rays: byte-identical hits (test_raycast.py checks the x-fastest hits against the reference)
        O, D = _long_rays(N, 256, 17)
        hx = _cast(ex, gx.data_ptr(), (N, N, N), sx, (0, 0, 0), 1.0, O, D)
        hz = _cast(ex, gz.data_ptr(), (N, N, N), sz, (0, 0, 0), 1.0, O, D)
        assert hx.tobytes() == hz.tobytes(), "x-fastest and z-fastest grids give different hits"
        assert (hx["triangle"] >= 0).sum() > 128

        # exact mode: the two layouts byte for byte
        ex.set_tuning(emit_fast_math=0)
        T, tris, offs = soup_on_device(ex, gx, sx)
        assert T == T_1026
        tx, ox = tris.clone(), offs.clone()
        T, tris, offs = soup_on_device(ex, gz, sz)
        assert T == T_1026
        assert torch.equal(offs, ox), "block offsets differ between the layouts"
        assert torch.equal(tris, tx), "exact-mode records differ between the layouts"
        # the comparisons bite: one flipped bit in a block with bx = 127, one triangle dropped from an offsets copy
        b = int(NB - 1 + NB * (NB // 2 + NB * (NB // 2)))
        assert int(ox[b + 1]) > int(ox[b]), "the probe block is empty"
        k = int(ox[b]) * ROW + 3
        tx.view(-1)[k] ^= 1
        assert not torch.equal(tris, tx)
        tx.view(-1)[k] ^= 1
        assert torch.equal(tris, tx)
        short = ox.clone()
        short[b + 1:] -= 1
        assert not torch.equal(offs, short)
        del short

        # the z-fastest grid on the host, blocks against the oracle (64-bit gather)
        hzh = host_copy_z(gz)
        blocks = far_face_blocks()
        ids = ids_of(blocks)
        want, want_offs, _ = oracle_mod.extract_grid(hzh, blocks, threads=8)
        rows, cnt = rows_of(tris, ROW, offs, ids)
        check_blocks_against_oracle(rows, cnt, want, want_offs, ids, "exact soup, z fastest")
        del rows, cnt, want, hzh

        # fast mode: offsets and ids of the exact run, floats within 2e-6; the layouts agree byte for byte
        ex.set_tuning(emit_fast_math=1)
        T, tris, offs = soup_on_device(ex, gx, sx)
        assert T == T_1026 and torch.equal(offs, ox)
        ids_ok, nan_ok, worst = float_gap(tris, tx)
        assert ids_ok and nan_ok and worst <= FAST_ATOL, (ids_ok, nan_ok, worst)
        fx = tris.clone()
        del tx
        T, tris, offs = soup_on_device(ex, gz, sz)
        assert T == T_1026 and torch.equal(offs, ox)
        assert torch.equal(tris, fx), "fast-mode records differ between the layouts"
        del fx, tris, offs, ox
    finally:
        ex.set_tuning(emit_fast_math=1)
        ex.close()
        free_gpu()


@pytest.mark.gpu
def test_csharp_array_1026_indexed_on_the_device(oracle_mod):
    """Indexed output in exact mode at 1026^3: the z-fastest grid gives the x-fastest grid's vertex and triangle counts, both offset
    arrays and byte-identical vertex and index buffers; the far-face block set equals oracle.extract_grid_indexed exactly."""
    import torch
    import volumetricterrain_amd as vt
    ex = vt.Extractor(0)
    try:
        ex.set_tuning(emit_fast_math=0)
        ex.set_output_mode(True)
        res = {}
        for order in ("x", "z"):
            g, strides = fill_1026(ex, order)
            T = ex.extract_volumes_device(g.data_ptr(), (N, N, N), strides, 1, 0)
            nv = ex.last_vertex_count()
            vp, ip, vop, top = ex.device_indexed_results()
            res[order] = (T, nv, device_view_i32(vp, 6 * nv).clone(), device_view_i32(ip, 3 * T).clone(),
                          device_view_i32(vop, NB ** 3 + 1).clone(), device_view_i32(top, NB ** 3 + 1).clone())
            if order == "z":
                hzh = host_copy_z(g)
            del g
            free_gpu()
        (Tx, nvx, vx, ix, vox, tox), (Tz, nvz, vz, iz, voz, toz) = res["x"], res["z"]
        assert Tx == Tz == T_1026 and nvx == nvz
        assert torch.equal(vox, voz) and torch.equal(tox, toz)
        assert torch.equal(vx, vz), "vertex buffers differ between the layouts"
        assert torch.equal(ix, iz), "index buffers differ between the layouts"
        del res, vx, ix, vox, tox

        blocks = far_face_blocks()
        ids = ids_of(blocks)
        wv, wi, wvo, wto = oracle_mod.extract_grid_indexed(hzh, blocks)
        del hzh
        verts, vcnt = rows_of(vz, 6, voz, ids)
        idx, tcnt = rows_of(iz, 3, toz, ids)
        assert np.array_equal(vcnt.cpu().numpy(), np.diff(wvo)) and np.array_equal(tcnt.cpu().numpy(), np.diff(wto))
        assert np.array_equal(idx.cpu().numpy(), wi)
        got = verts.cpu().numpy().view(np.float32)
        want = np.concatenate([wv["position"], wv["normal"]], axis=1)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(float_bits(got), float_bits(want)), "indexed vertices differ from the oracle's"
    finally:
        ex.set_output_mode(False)
        ex.set_tuning(emit_fast_math=1)
        ex.close()
        free_gpu()


# ---- 3. the C# array at full size, through the host entry points ---------------------------------------------------------------

@pytest.mark.gpu
def test_csharp_array_1026_through_the_host_entry_points(oracle_mod):
    """The literal INTEGRATION.md route: a host float[,,] of 1026^3 samples (z fastest, 4.3 GB) through the three branches of
    vtmc_extract_grid -- no block list (upload, dense z-lane classify), a small dirty list (host tile gather with sz < sx) and a
    checkerboard of half the blocks (upload, device block list) -- and through vtmc_extract_grid_sharded.  Exact mode; the
    reference is the x-fastest device extract of the same field and the oracle."""
    import torch
    import volumetricterrain_amd as vt
    ex = vt.Extractor(0)
    try:
        ex.set_tuning(emit_fast_math=0)
        gx, sx = fill_1026(ex, "x")
        T, tris, offs = soup_on_device(ex, gx, sx)
        assert T == T_1026
        tx, ox = tris.clone(), offs.clone()
        del gx, tris, offs
        gz, _ = fill_1026(ex, "z")
        hz = host_copy_z(gz)
        del gz
        free_gpu()
        assert hz.strides == (4 * DIM * DIM, 4 * DIM, 4)
        counts = np.diff(ox.cpu().numpy().astype(np.int64))
        blocks_far = far_face_blocks()

        # 1. no block list
        assert ex.extract_grid(hz) == T_1026
        tri_ptr, off_ptr, _ = ex.device_results()
        assert torch.equal(device_view_i32(off_ptr, NB ** 3 + 1), ox)
        assert torch.equal(device_view_i32(tri_ptr, T_1026 * ROW).view(-1, ROW), tx), "host route records differ"

        # 2. a small dirty list: every block with bx = by = 127 (the far corner among them) and random others, shuffled
        rng = np.random.default_rng(9)
        col = np.stack([np.full(NB, NB - 1), np.full(NB, NB - 1), np.arange(NB)], 1)
        small = np.concatenate([col, rng.integers(0, NB, size=(300 - NB, 3))]).astype(np.int32)
        small = small[rng.permutation(len(small))]
        assert len(small) * 2000 < host_span(hz)
        T = ex.extract_grid(hz, small)
        got, got_offs = ex.read_triangles()
        want, want_offs, _ = oracle_mod.extract_grid(hz, small, threads=8)
        assert T == len(want) and np.array_equal(got_offs, want_offs)
        assert_soup(got, want, exact=True, what="small dirty list")
        assert np.array_equal(np.diff(want_offs), counts[ids_of(small)])

        # 3. a checkerboard: more blocks than span / 2000, so the grid is uploaded and the list goes to the device
        allb = oracle_mod.all_blocks(N, N, N)
        cb = allb[allb.sum(axis=1) % 2 == 0]
        assert len(cb) * 2000 >= host_span(hz)
        cb_ids = ids_of(cb)
        T = ex.extract_grid(hz, cb)
        assert T == counts[cb_ids].sum()
        tri_ptr, off_ptr, _ = ex.device_results()
        got_offs = device_view_i32(off_ptr, len(cb) + 1).cpu().numpy()
        assert np.array_equal(got_offs, np.concatenate([[0], np.cumsum(counts[cb_ids])]))
        lib_tris = device_view_i32(tri_ptr, T * ROW)
        ref_rows, ref_cnt = rows_of(tx.view(-1), ROW, ox, cb_ids)
        got_rows = lib_tris.view(-1, ROW)
        assert torch.equal(got_rows[:, :18], ref_rows[:, :18]), "checkerboard records differ from the x-fastest device extract"
        # a listed block's records carry its position in the list, the whole grid's its canonical id
        assert torch.equal(got_rows[:, 18], torch.repeat_interleave(torch.arange(len(cb), device=ref_cnt.device, dtype=torch.int32), ref_cnt))
        del ref_rows, ref_cnt, got_rows
        on = blocks_far[blocks_far.sum(axis=1) % 2 == 0]
        pos = np.searchsorted(cb_ids, ids_of(on))
        assert np.array_equal(cb_ids[pos], ids_of(on)) and len(on) > 20000
        rows, cnt = rows_of(lib_tris, ROW, device_view_i32(off_ptr, len(cb) + 1), pos)
        want, want_offs, _ = oracle_mod.extract_grid(hz, on, threads=8)
        check_blocks_against_oracle(rows, cnt, want, want_offs, pos, "checkerboard")
        del rows, cnt, lib_tris, want, tx

        # sharded: 512 chunks of 128^3, world 2 -- chunk c = cx + 8 (cy + 8 cz) belongs to rank c % 2
        k = 128 // 8
        per_chunk = counts.reshape(NB // k, k, NB // k, k, NB // k, k).sum(axis=(1, 3, 5)).reshape(-1)
        total = 0
        for rank in range(2):
            T, cc = ex.extract_grid_sharded(hz, 128, rank, 2)
            assert len(cc) == 256
            assert np.array_equal(cc[:, 1].astype(np.int64), per_chunk[rank::2]), rank
            assert np.array_equal(cc[:, 0], 3 * cc[:, 1])
            assert T == cc[:, 1].sum()
            total += T
        assert total == T_1026
    finally:
        ex.set_tuning(emit_fast_math=1)
        ex.close()
        free_gpu()
