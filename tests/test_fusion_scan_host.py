"""CPU: the host-only side of the scan-level fusion path -- the pair table the scan launches index a scan's maps with
(``ops.fusion_pair_table`` = ``fusion.pair_table`` = ``dtu_fusion.pair_table``), built from the ``read_pair_file`` list without a GPU
and without the library, and the scan entries' place in the C ABI."""
import pytest
import torch

from effi_mvs_plus_amd import _lib, dtu_fusion, fusion, ops

PAIRS = [(0, [1, 2]), (1, [0, 2, 3]), (2, [0, 1, 3, 4, 5]), (3, [5, 4, 2, 1]), (5, [4, 3])]


def test_pair_table_rows_are_reference_then_sources_then_padding():
    t = fusion.pair_table(PAIRS)
    assert t.dtype == torch.int32 and not t.is_cuda and t.is_contiguous() and tuple(t.shape) == (5, 6)
    assert t.tolist() == [[0, 1, 2, -1, -1, -1], [1, 0, 2, 3, -1, -1], [2, 0, 1, 3, 4, 5], [3, 5, 4, 2, 1, -1], [5, 4, 3, -1, -1, -1]]
    assert torch.equal(t, dtu_fusion.pair_table(PAIRS)) and torch.equal(t, ops.fusion_pair_table(PAIRS))
    # source order is kept (the averaged depth sums the sources in list order), a reference view may appear twice
    assert fusion.pair_table([(4, [9, 0]), (4, [0, 9])]).tolist() == [[4, 9, 0], [4, 0, 9]]
    # the 16-source limit belongs to the kernels, not to the table: 17 sources build a table the scan entries then refuse
    assert tuple(fusion.pair_table([(0, list(range(1, 18)))]).shape) == (1, 18)


def test_pair_table_reads_what_read_pair_file_returns(tmp_path):
    with open(tmp_path / "pair.txt", "w") as f:
        f.write("3\n0\n2 1 90.5 2 80.0\n1\n0\n2\n1 0 70.0\n")
    data = dtu_fusion.read_pair_file(str(tmp_path / "pair.txt"))
    assert data == [(0, [1, 2]), (2, [0])]                       # view 1 has no sources: read_pair_file skips it
    assert fusion.pair_table(data).tolist() == [[0, 1, 2], [2, 0, -1]]


@pytest.mark.parametrize("bad", [[], [(0, [])], [(-1, [1])], [(0, [1, -2])]])
def test_pair_table_refuses_what_no_launch_could_use(bad):
    with pytest.raises(ValueError):
        fusion.pair_table(bad)


def test_scan_entries_are_declared_and_bound():
    names = {"effi_fusion_dtu_filter_scan_f32", "effi_fusion_dynamic_filter_scan_f32", "effi_fusion_compact_blocks",
             "effi_fusion_compact_scan_tile", "effi_fusion_compact_count_u8", "effi_fusion_compact_scatter_f32"}
    assert names <= set(_lib.SIGNATURES) and names <= set(_lib.declared_symbols())
    for fn in (ops.fusion_dtu_filter_scan, ops.fusion_dynamic_filter_scan, ops.fusion_compact, dtu_fusion.fuse_scan,
               fusion.dynamic_filter_scan):
        assert callable(fn)


def test_scan_wrappers_refuse_cpu_tensors():
    d, cams = torch.zeros(3, 8, 8), torch.zeros(3, 2, 4, 4)
    with pytest.raises(_lib.EffiLibraryError):
        ops.fusion_dtu_filter_scan(d, cams, fusion.pair_table([(0, [1, 2])]))
    with pytest.raises(_lib.EffiLibraryError):
        ops.fusion_dynamic_filter_scan(d, cams, fusion.pair_table([(0, [1, 2])]))
