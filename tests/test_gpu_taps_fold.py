"""The three taps families (Tracer.taps, array_taps, beam_taps) share one sinc GEMM body (csrc/hrt_taps_gemm.inc), one
tap grid (hrt_ktgrid, taps_grid() of csrc/host/channel.c) and one reduce / launch (csrc/hrt_pathsum.h).  Against what
the build before that fold gave, recorded in tests/golden/taps_fold.json (tests/taps_fold_util.py says how):

  the host plan   every scratch size of TF.plan_cases() is the recorded one.  The size holds the chunk count, which is
                  ceil(2048 / (links * rblocks * cblocks)) in these cases, so a wrong rblocks or cblocks shows: the
                  two sides of the rows 64 / 65 and taps 64 / 65 edges (and the others listed there) are asserted to
                  give different chunk counts.
  the outputs     the sha256 of the raw output bytes of every case of TF.output_cases(), written plainly and then
                  accumulated once, is the recorded one: both forms of each family, with and without the LoS part, on
                  a planted workspace.  The kernels promise the same bits for the same inputs (no float atomics, the
                  chunks added in a fixed order)."""
import pytest

from . import taps_fold_util as TF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tracer():
    tr = TF.planted_tracer()
    yield tr
    tr.close()


@pytest.fixture(scope="module")
def golden():
    return TF.golden()


def test_scratch_sizes_are_the_recorded_ones(tracer, golden):
    want = golden["scratch_bytes"]
    got = TF.plan_sizes(tracer)
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, "scratch sizes (got, recorded): %r" % bad


# (family, rows or taps edge, the other size): the two sides must plan different chunk counts
EDGES = [("taps", "rows", (16, 17), 17), ("array_taps", "rows", (64, 65), 17), ("beam_taps", "rows", (64, 65), 17),
         ("taps", "rows", (12, 13), 17), ("array_taps", "rows", (12, 13), 17), ("beam_taps", "rows", (12, 13), 17),
         ("taps", "L", (64, 65), 13), ("array_taps", "L", (64, 65), 13), ("beam_taps", "L", (64, 65), 13),
         ("taps", "L", (256, 257), 4), ("array_taps", "L", (256, 257), 4), ("beam_taps", "L", (256, 257), 4)]


@pytest.mark.parametrize("fam,axis,edge,other", EDGES)
def test_an_edge_changes_the_chunk_count(tracer, golden, fam, axis, edge, other):
    """what makes the size comparison see rblocks and cblocks: across an edge of the tiling the chunk count differs,
    and both sides are the recorded sizes"""
    n = []
    for v in edge:
        rows, L = (v, other) if axis == "rows" else (other, v)
        shape = (1, 1, rows) if fam == "taps" else TF.PAIR_ROWS[rows]
        for shard in TF.SHARDS:
            need, chunks = TF.scratch_bytes(tracer, fam, shape, L, "both", shard)
            assert need == golden["scratch_bytes"]["%s rows%d L%d both %s" % (fam, rows, L, shard)]
            assert chunks >= 2, (fam, rows, L, shard, chunks)
        n.append(chunks)
        assert TF.scratch_bytes(tracer, fam, shape, L, "los", "1of1")[1] == 0   # LoS only: no partial sums
    print("%s %s %r: chunks %r" % (fam, axis, edge, n))
    assert n[0] != n[1], (fam, axis, edge, n)


@pytest.mark.parametrize("key,fam,shape,los", list(TF.output_cases()), ids=[c[0] for c in TF.output_cases()])
def test_output_bytes_are_the_recorded_ones(tracer, golden, key, fam, shape, los):
    first, second = TF.output_hashes(tracer, fam, shape, los)
    assert first != second   # the accumulated call added something
    assert (first, second) == (golden["sha256"][key], golden["sha256"][key + " accumulated"]), key
