"""volumetricterrain_amd/_header.py reads include/vtmc.h, and the ctypes binding is built from what it reads.  These tests pin the reader
against literals taken from the header as it stands (not from the reader): prototypes, struct layouts, constants -- and its strictness:
a form it does not know raises, naming the line; nothing is skipped."""
import ctypes
import os

import pytest

from volumetricterrain_amd import _header, _lib

H = _header.HEADER
VP, I32, U32, I64, U64, F32, STR = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float,
                                    ctypes.c_char_p)


def test_the_reader_reads_the_header_the_build_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.samefile(_header.PATH, os.path.join(root, "include", "vtmc.h"))


def test_prototypes():
    p = H.prototypes
    assert len(p) == 77   # a condition: update it when the header grows
    assert p["vtmc_terrain_init"].argtypes == [VP, I32, I32, I32, F32, VP, U64] and p["vtmc_terrain_init"].restype is I32
    fill = p["vtmc_density_fill_device"].argtypes
    assert len(fill) == 13 and fill[7:11] == [I64] * 4 and fill[3:7] == [I32] * 4 and fill[:3] == [VP] * 3 and fill[11:] == [VP] * 2
    assert p["vtmc_density_fill_device_async"].argtypes == fill
    mesh = p["vtmc_stamp_from_mesh"].argtypes
    assert len(mesh) == 12 and mesh[6] is F32 and mesh[10] is U32 and mesh == [VP, VP, I32, VP, I32, VP, F32, I32, I32, I32, U32, VP]
    assert p["vtmc_chunk_write"].argtypes == [VP, STR, I32, VP, I32]
    assert p["vtmc_set_tuning"].argtypes == [VP, STR, I32]
    assert p["vtmc_last_error"].restype is STR and p["vtmc_last_error"].argtypes == [VP]
    assert p["vtmc_release_streams"].argtypes == [] and p["vtmc_release_streams"].restype is I32
    assert p["vtmc_version"].argtypes == [] and p["vtmc_version"].restype is STR
    assert p["vtmc_last_stage_ms"].argtypes == [VP, VP]                 # float ms[4]: an array parameter is a pointer
    assert p["vtmc_comm_unique_id"].argtypes == [VP]                    # uint8_t id[VTMC_COMM_ID_BYTES]
    assert p["vtmc_device_results"].argtypes == [VP, VP, VP, VP]        # const vtmc_triangle **: any depth of pointer
    assert p["vtmc_terrain_history"].argtypes == [VP, VP, VP, VP]
    assert p["vtmc_terrain_set_history"].argtypes == [VP, I64]
    assert p["vtmc_extract_blocks"].ret == "int32_t" and p["vtmc_extract_blocks"].params == [
        "vtmc_ctx *ctx", "const float *samples", "int32_t n_blocks", "int32_t *tri_count"]
    assert _lib.SYMBOLS == list(p)


# struct: (bytes, last field, its offset)
LAYOUTS = {"vtmc_triangle": (76, "block", 72), "vtmc_vertex": (24, "normal", 12), "vtmc_ray_hit": (56, "triangle", 52),
           "vtmc_sphere_hit": (48, "triangle", 44), "vtmc_instance": (32, "rnd", 28), "vtmc_fragment": (48, "reserved", 44),
           "vtmc_modifier": (80, "data_dims", 72), "vtmc_material_stroke": (24, "channel", 20), "vtmc_ao_params": (16, "flags", 12),
           "vtmc_scatter_params": (36, "flags", 32), "vtmc_lod_params": (24, "max_nodes", 20), "vtmc_lod_node": (16, "level", 12),
           "vtmc_volume_batch": (64, "volume_stride", 56), "vtmc_chunk_view": (88, "d_indices", 80),
           "vtmc_density_params": (32, "ramp_center", 28)}
WITH_POINTERS = {"vtmc_modifier", "vtmc_volume_batch", "vtmc_chunk_view"}


def test_struct_layouts():
    assert set(H.structs) == set(LAYOUTS)
    for name, (size, last, offset) in LAYOUTS.items():
        s = H.structure(name, "S")
        assert ctypes.sizeof(s) == size, name
        assert s._fields_[-1][0] == last and getattr(s, last).offset == offset, name
        if name in WITH_POINTERS:
            with pytest.raises(_header.HeaderError):
                H.dtype(name)
        else:
            d = H.dtype(name)
            assert d.itemsize == size and d.names[-1] == last and d.fields[last][1] == offset, name
            assert d.names == tuple(f for f, _ in s._fields_) and all(d.fields[f][1] == getattr(s, f).offset for f in d.names), name
            assert all(d.fields[f][0].base.byteorder in "<=" for f in d.names), name


def test_struct_fields_in_every_form_the_header_uses():
    vb = H.structure("vtmc_volume_batch", "VB")
    assert vb._fields_ == [("d_samples", VP), ("nx", I32), ("ny", I32), ("nz", I32), ("stride_x", I64), ("stride_y", I64),
                           ("stride_z", I64), ("n_volumes", I32), ("volume_stride", I64)]
    assert vb.stride_x.offset == 24            # natural alignment: four bytes of padding after nz
    m = H.structure("vtmc_modifier", "M")
    assert m.p.offset == 32 and m.p.size == 32 and m.data.offset == 64
    assert H.structure("vtmc_density_params", "D")._fields_[0] == ("seed", U64)
    assert _lib.AoParams(1.0, 1.0, 4, 0).steps == 4 and _lib.AoParams.__name__ == "AoParams"   # positional construction
    assert _lib.TRI_DTYPE.names == ("p0", "p1", "p2", "n0", "n1", "n2", "block") and _lib.TRI_DTYPE.fields["n2"][1] == 60
    assert _lib.TRI_DTYPE.itemsize == 76 and _lib.TRI_DTYPE["p0"].shape == (3,)


def test_constants():
    c = H.constants
    assert "VTMC_H" not in c
    assert c["VTMC_ERR_TOO_LARGE"] == -6 and _lib.ERR_TOO_LARGE == -6
    assert c["VTMC_MESH_MAX_TRIANGLES"] == 1 << 20 and _lib.MESH_MAX_TRIANGLES == 1 << 20
    assert c["VTMC_MESH_BAND"] == 3.0 and isinstance(_lib.MESH_BAND, float)
    assert c["VTMC_SCATTER_MAX_DENSITY_CELLS"] == 8.0 and isinstance(_lib.SCATTER_MAX_DENSITY_CELLS, float)
    assert c["VTMC_FLAG_NO_DENSE_PATH"] == 2 and isinstance(_lib.FLAG_NO_DENSE_PATH, int)
    assert (_lib.OK, _lib.ERR_INVALID_ARG, _lib.MOD_DETACH, _lib.COMM_ID_BYTES, _lib.TILE_SAMPLES) == (0, -1, 11, 128, 1000)


ALTERATIONS = [   # (what, the line as it stands, the line instead, the line the error names relative to it)
    ("a parameter of an unknown type", "int32_t vtmc_destroy(vtmc_ctx *ctx);", "int32_t vtmc_destroy(vtmc_ctx *ctx, double x);", 0),
    ("a pointer to an unknown type", "int32_t vtmc_destroy(vtmc_ctx *ctx);", "int32_t vtmc_destroy(vtmc_context *ctx);", 0),
    ("a value of a struct type", "int32_t vtmc_destroy(vtmc_ctx *ctx);", "int32_t vtmc_destroy(vtmc_ctx *ctx, vtmc_vertex v);", 0),
    ("a #define that is no literal", "#define VTMC_OK 0", "#define VTMC_X sizeof(int)", 0),
    ("a prototype returning double", "const char *vtmc_version(void);", "double vtmc_version(void);", 0),
    ("a call that is no prototype", "const char *vtmc_version(void);", "static int v = vtmc_version(1)[0];", 0),
    ("a prototype declared twice", "const char *vtmc_version(void);", "int32_t vtmc_comm_destroy(vtmc_ctx *ctx);", 0),
    ("a function-like macro", "#define VTMC_OK 0", "#define VTMC_CALL(x) vtmc_destroy(x)", 0),
    ("a field of an unknown type", "    int32_t level;", "    int16_t level;", 0),
    ("a struct in a struct", "    int32_t level;", "    struct { int32_t a; } level;", -2),
]


@pytest.mark.parametrize("what,line,instead,named", ALTERATIONS, ids=[a[0].replace(" ", "_") for a in ALTERATIONS])
def test_the_reader_raises_on_what_it_does_not_know(tmp_path, what, line, instead, named):
    lines = open(_header.PATH).read().split("\n")
    assert lines.count(line) == 1, line
    at = lines.index(line)
    lines[at] = instead
    path = tmp_path / "vtmc.h"
    path.write_text("\n".join(lines))
    with pytest.raises(_header.HeaderError) as e:
        _header.Header(str(path))
    assert "%s:%d:" % (path, at + 1 + named) in str(e.value), (what, str(e.value))


def test_an_unaltered_copy_reads_the_same(tmp_path):
    path = tmp_path / "vtmc.h"
    path.write_text(open(_header.PATH).read())
    h = _header.Header(str(path))
    assert h.constants == H.constants and list(h.structs) == list(H.structs)
    assert h.prototypes == H.prototypes
