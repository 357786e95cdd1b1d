"""What the host tests of the section modules (test_fremlp_cabi, test_sfh_fu_cabi, test_sfh_ffn_cabi, test_sfh_mixer_cabi,
test_bn2d_cabi) ask of every ``sections`` / ``saved_sections`` map of a plan."""


def up256(n: int) -> int:
    return -(-n // 256) * 256


def sections_tile(sections: dict, unplaced_empty: bool = False):
    """Asserts that the name -> (byte offset, bytes) sections start on 256-byte boundaries, lie in order and do not overlap.
    ``unplaced_empty``: an empty section may sit at offset 0 (a mode that does not use a section leaves it there).
    -> (where the last section ends, the sum of the sizes each rounded up to 256): the caller holds them against the totals."""
    end = total = 0
    for name, (off, nbytes) in sections.items():
        assert off % 256 == 0 and (off >= end or (unplaced_empty and nbytes == 0)), name
        end, total = max(end, off + nbytes), total + up256(nbytes)
    return end, total
