"""The host half of io.Pod5Dataset / io.open_pod5 (a run's directory of POD5 files where the reference hands the argument to
pod5.DatasetReader, src/remora/io.py:427): which files a directory names, the addressing of reads by global row, the refusals.
Nothing here touches the GPU - the read-id index is built when an id is first asked for (tests/test_gpu_pod5_dataset.py)."""
import os
import shutil

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")
CAN, MOD = os.path.join(DATA, "can_reads.pod5"), os.path.join(DATA, "mod_reads.pod5")


def test_a_directory_names_its_pod5_files_sorted_and_not_recursively(tmp_path):
    from remora_amd import io as rio

    run = tmp_path / "run"
    (run / "sub").mkdir(parents=True)
    for name in ("b.pod5", "a.pod5", "sub/c.pod5"):
        shutil.copy(CAN, run / name)
    os.symlink(MOD, run / "0_link.pod5")
    shutil.copy(os.path.join(DATA, "duplex_reads.pod5.part00"), run / "duplex_reads.pod5.part00")
    (run / "notes.txt").write_text("not signal")
    (run / "dir.pod5").mkdir()  # a directory is no file, whatever its name
    want = [str(run / n) for n in ("0_link.pod5", "a.pod5", "b.pod5")]
    assert rio.list_pod5_files(run) == want
    assert rio.list_pod5_files(str(run) + os.sep) == [os.path.join(str(run) + os.sep, os.path.basename(p)) for p in want]
    ds = rio.open_pod5(str(run))
    assert isinstance(ds, rio.Pod5Dataset) and ds.paths == want and ds.n_rows == 3 * 14
    assert rio.open_pod5(ds) is ds
    # a list keeps the caller's order; a directory inside it is listed by the rule
    ds2 = rio.open_pod5([MOD, str(run)])
    assert ds2.paths == [MOD] + want


def test_open_pod5_of_a_file_is_the_pod5_file_it_always_was():
    from remora_amd import io as rio

    f = rio.open_pod5(CAN)
    assert type(f) is rio.Pod5File and len(f) == 14 and len(f.read_ids) == 14 and set(f._row) == set(f.read_ids)
    assert rio.open_pod5(f) is f
    assert not hasattr(f, "rows_of_names")  # the batch ingest keeps its dictionary for a single file


def test_members_keep_no_descriptor_and_make_no_per_read_objects(tmp_path):
    from remora_amd import io as rio

    before = len(os.listdir("/proc/self/fd"))
    ds = rio.Pod5Dataset([CAN, MOD, CAN])
    assert len(os.listdir("/proc/self/fd")) == before
    for f in ds.files:
        assert not hasattr(f, "_fh") and not hasattr(f, "read_ids") and not hasattr(f, "_row")
    assert ds._ids is None and ds._index is None
    # the keys of the index: views of the mapped files, 16 bytes a read, equal to the ids the single-file reader lists
    import uuid

    views = [v for f in ds.files for v in f._read_id_bytes()]
    assert all(v.dtype == np.uint8 and v.shape[1] == 16 and not v.flags.owndata and not v.flags.writeable for v in views)
    ids = [str(uuid.UUID(bytes=row.tobytes())) for v in views for row in v]
    assert ids == rio.Pod5File(CAN).read_ids + rio.Pod5File(MOD).read_ids + rio.Pod5File(CAN).read_ids
    assert ds.read_ids == ids


def test_rows_of_reads_by_global_row_equals_the_files_own(tmp_path):
    from remora_amd import io as rio

    ds = rio.Pod5Dataset([CAN, MOD])
    single = [rio.Pod5File(CAN), rio.Pod5File(MOD)]
    assert ds._first.tolist() == [0, 14, 28]
    assert np.array_equal(ds._cal_off, np.concatenate([f._cal_off for f in single]))
    assert np.array_equal(ds._cal_scale, np.concatenate([f._cal_scale for f in single]))
    rng = np.random.default_rng(5)
    orders = [np.arange(28), np.arange(28)[::-1], rng.permutation(28), np.asarray([27, 0, 14, 13, 0, 27]), np.asarray([3]), np.asarray([20, 21]),
              np.zeros(0, np.int64)]
    for rows in orders:
        first, addr, size, samples = ds.rows_of_reads(rows)
        assert first.dtype == np.int64 and addr.dtype == np.uint64 and size.dtype == np.int64 and samples.dtype == np.int64
        assert first.size == rows.size + 1 and first[0] == 0 and addr.size == size.size == samples.size == first[-1]
        for k, r in enumerate(rows.tolist()):
            f, local = (0, r) if r < 14 else (1, r - 14)
            w_first, w_addr, w_size, w_samples = single[f].rows_of_reads([local])
            got = slice(int(first[k]), int(first[k + 1]))
            assert np.array_equal(size[got], w_size) and np.array_equal(samples[got], w_samples)
            # absolute addresses into ANOTHER mapping of the same file: the bytes they point at are the same
            import ctypes

            for a, b, n in zip(addr[got].tolist(), w_addr.tolist(), w_size.tolist()):
                assert ctypes.string_at(a, n) == ctypes.string_at(b, n)
    for bad in ([28], [-1], [0, 99]):
        with pytest.raises(rio.RemoraError, match="row out of range"):
            ds.rows_of_reads(bad)


def test_refusals_name_the_directory_and_the_file(tmp_path):
    from remora_amd import io as rio

    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "reads.pod5.part00").write_bytes(b"x")
    with pytest.raises(rio.RemoraError) as e:
        rio.open_pod5(str(empty))
    assert str(e.value) == f"no *.pod5 files in directory {empty}"
    text = tmp_path / "text"
    text.mkdir()
    (text / "reads.pod5").write_text("these are not the reads you are looking for\n")
    with pytest.raises(rio.RemoraError) as e:
        rio.open_pod5(str(text))
    assert str(e.value) == f"{text / 'reads.pod5'} is not a POD5 file"
    with pytest.raises(rio.RemoraError) as e:  # the single-file route says the same, as before
        rio.open_pod5(str(text / "reads.pod5"))
    assert str(e.value) == f"{text / 'reads.pod5'} is not a POD5 file"
    (text / "void.pod5").write_bytes(b"")
    with pytest.raises(rio.RemoraError) as e:
        rio.open_pod5([str(text / "void.pod5")])
    assert str(e.value) == f"{text / 'void.pod5'} is not a POD5 file"
