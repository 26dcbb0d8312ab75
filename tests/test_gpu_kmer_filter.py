"""fsv_asm_params.kmer_filter = 1 through fsv_assemble_batch: hifiasm's high-count k-mer filter in every sketch of the assembly.
 - the option needs kmer_table = 1;
 - where the filter is empty nothing may move: contigs, corrected reads and statuses byte for byte those of kmer_filter = 0;
 - the sets without a coverage peak come back as with kmer_table = 1 alone (left alone, flagged);
 - the 21 repeat-rich golden sets whose filter is not empty, after three rounds with both options on, against the corrected reads and
   contigs hifiasm-0.14 itself wrote (tests/golden/hifiasm_repeats.json; hifiasm ran with its filter on).  A set that differs is listed in
   KNOWN_FILTER_DEVIATIONS with its cause, and the test asserts both ways."""
import hashlib
import json
import os

import pytest

from focalsv_amd import _lib, synth
from focalsv_amd.readsets import pack_sets
from tests import kmer_model as KM
from tests.test_oracle_asm import check_repeat_set

pytestmark = pytest.mark.gpu

# repeat set index -> cause, traced in the reference's code.  At most 3 of the 21 (the project's scale for such lists).
KNOWN_FILTER_DEVIATIONS = {}


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def assemble(ctx, sets, kmer_table, kmer_filter):
    b = pack_sets(sets)
    d = ctx.upload(b.words)
    try:
        p = ctx.default_asm_params()
        p.kmer_table, p.kmer_filter = kmer_table, kmer_filter
        contigs, cset, cnr, status = ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
        reads = ctx.fetch_reads(b.n_reads, int(b.read_len.sum()) * 2 + 1024)
    finally:
        ctx.dev_free(d)
    per_set, per_reads, k = [], [], 0
    for s in range(len(sets)):
        per_set.append([c for c, cs in zip(contigs, cset) if cs == s])
        per_reads.append(reads[k:k + len(sets[s])])
        k += len(sets[s])
    return per_set, per_reads, [int(x) for x in status]


def test_filter_needs_the_table(ctx):
    r = synth.make_region(700, width=26000, depth_per_hap=6.0)
    b = pack_sets([r.reads[1]])
    d = ctx.upload(b.words)
    try:
        p = ctx.default_asm_params()
        p.kmer_filter = 1
        with pytest.raises(_lib.FsvError) as e:
            ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
        assert e.value.code == _lib.EINVAL and "kmer_filter" in str(e.value) and "kmer_table" in str(e.value)
    finally:
        ctx.dev_free(d)


@pytest.fixture(scope="module")
def table_gold(golden_dir):
    return json.load(open(os.path.join(golden_dir, "hifiasm_kmer_table.json")))["sets"]


def test_empty_filters_and_missing_peaks_change_nothing(ctx, table_gold):
    """two phased sets with a peak and an empty filter, and the four sets without a peak, in one call: kmer_filter = 1 gives the bytes of
    kmer_filter = 0 (both with kmer_table = 1) -- the sets without a peak uncorrected, without a contig, flagged"""
    phased = [g for g in table_gold if g["kind"] == "lowcov" and g["ft"]["filtered"] == 0][:2]
    none = [g for g in table_gold if g["ft"]["cutoff"] < 0]
    assert len(phased) == 2 and len(none) == 4
    recs = [none[0], phased[0], none[1], none[2], phased[1], none[3]]
    sets = [KM.reads_of(g) for g in recs]
    with1 = assemble(ctx, sets, 1, 1)
    with0 = assemble(ctx, sets, 1, 0)
    assert with1 == with0
    contigs, reads, status = with1
    for s, g in enumerate(recs):
        if g["ft"]["cutoff"] < 0:
            assert status[s] & _lib.W_LOW_COV and status[s] & _lib.W_NO_LAYOUT and contigs[s] == [] and reads[s] == list(sets[s]), s
        else:
            assert not status[s] & _lib.W_LOW_COV and len(contigs[s]) >= 1 and reads[s] != list(sets[s]), s


def test_the_assembly_sketches_through_the_filter(ctx, golden_dir):
    """repeat set 9 (2 656 filtered k-mers) with no correction round: the final pass sketches the raw reads, and the minimizers its sketch
    kernel produced (fsv_asm_stats charges the kernel 16 B for each) are the filtered sketch's -- fewer than the plain sketch's by what the
    model says -- so the pipeline's own launch takes the filter sets, not only the index stage"""
    from tests import sketch_filter_model as FM
    reads = synth.make_repeat_region(9).reads[0]
    _, midx = FM.kmer_index(reads, 51, 51, 1)
    plain = KM.kmer_table(reads, 51)["n_entries"]
    assert midx["n_entries"] != plain
    b = pack_sets([reads])
    d = ctx.upload(b.words)
    produced = {}
    try:
        for kf in (0, 1):
            p = ctx.default_asm_params()
            p.kmer_table, p.kmer_filter, p.n_rounds = 1, kf, 0
            ctx.assemble_batch(d, b.word_off, b.read_len, b.set_start, p)
            produced[kf] = ctx.asm_stats()["kernels"]["k_sketch"]["algo_bytes"]
            if kf:
                idx, _ = ctx.last_kmer_index(1)
                assert int(idx[0]["n_entries"]) == midx["n_entries"]
    finally:
        ctx.dev_free(d)
    assert produced[0] - produced[1] == 16 * (plain - midx["n_entries"]), (produced, plain, midx["n_entries"])


# ---- the repeat-rich sets: hifiasm's own corrected reads and contigs -----------------------------------------------------------
def _filtered_repeat_sets():
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "hifiasm_kmer_table.json")))["sets"]
    return [g["index"] for g in gold if g["kind"] == "repeat" and g["ft"]["filtered"] > 0]


FILTERED = _filtered_repeat_sets()


@pytest.fixture(scope="module")
def repeats(ctx, golden_dir):
    """the 21 sets in one fsv_assemble_batch call (three rounds, kmer_table = 1, kmer_filter = 1)"""
    gold = {g["index"]: g for g in json.load(open(os.path.join(golden_dir, "hifiasm_repeats.json")))["sets"]}
    regions = {i: synth.make_repeat_region(i) for i in FILTERED}
    for i in FILTERED:
        assert hashlib.md5(b"\n".join(regions[i].reads[0])).hexdigest() == gold[i]["reads_md5"], "synthetic generator drifted"
    contigs, reads, status = assemble(ctx, [regions[i].reads[0] for i in FILTERED], 1, 1)
    return gold, regions, {i: (contigs[n], reads[n], status[n]) for n, i in enumerate(FILTERED)}


def test_the_list_is_short():
    assert len(FILTERED) == 21 and len(KNOWN_FILTER_DEVIATIONS) <= 3 and set(KNOWN_FILTER_DEVIATIONS) <= set(FILTERED)


@pytest.mark.parametrize("idx", FILTERED)
def test_filtered_repeat_sets_equal_hifiasm(repeats, idx):
    gold, regions, out = repeats
    contigs, reads, status = out[idx]
    g = gold[idx]
    assert "filtered out" in g["hifiasm_filter"]
    differs = False
    try:
        assert status == 0
        check_repeat_set(g, contigs, reads, regions[idx].haps[0])
    except AssertionError:
        if idx not in KNOWN_FILTER_DEVIATIONS:
            raise
        differs = True
    assert differs == (idx in KNOWN_FILTER_DEVIATIONS), (idx, "listed as a deviation, but equal to hifiasm")
