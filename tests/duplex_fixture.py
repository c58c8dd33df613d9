"""The duplex fixture files of tests/golden/data (the reference's tests/data/duplex_reads.pod5, simplex_reads_mapped.bam,
duplex_reads_mapped.bam, duplex_pairs.txt).  The POD5 is committed as two byte ranges (duplex_reads.pod5.part00 / .part01:
no tracked file above 1 MiB); duplex_pod5() writes them back to back."""
import os

from conftest import GOLDEN

DATA = os.path.join(GOLDEN, "data")
SIMPLEX_BAM = os.path.join(DATA, "simplex_reads_mapped.bam")
DUPLEX_BAM = os.path.join(DATA, "duplex_reads_mapped.bam")
PAIRS = os.path.join(DATA, "duplex_pairs.txt")


def duplex_pod5(tmp_dir):
    """Path of the joined POD5 file under `tmp_dir`."""
    path = os.path.join(str(tmp_dir), "duplex_reads.pod5")
    if not os.path.exists(path):
        with open(path, "wb") as out:
            for part in ("part00", "part01"):
                with open(os.path.join(DATA, f"duplex_reads.pod5.{part}"), "rb") as fh:
                    out.write(fh.read())
    return path
