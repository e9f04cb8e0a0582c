"""The core string functions on rows that cross every boundary of the wave-shaped string kernels, on the GPU: like /
ilike / regexp_like, the compares, IN, starts_with / ends_with, the lengths, locate / position / strpos, ascii, the
hashes, substr / left / right, the trims, castVARCHAR, upper / lower / initcap / reverse, replace, the pads, concat /
concatOperator, if over strings and their nestings — over the corpus of tests/string_shapes.py (row lengths 0..65613,
sub-tiles and wave tiles of T - 1, T and T + 1 bytes for every threshold of the kernels, in and out; needles on every
16- and 1024-byte boundary and split over rows, sub-tiles, wave tiles and a NULL row; runs of empty rows, NULL rows and
spaces) against its plain-Python reference, bit for bit.

Every family runs in fresh child processes with a time limit of their own (tests/full_range_child.py), the projectors
grouped as string_shapes.GROUP_SHAPES says: "wave" (ASCII text on the optimistic kernels, path_hint 0; multi-byte text
on the exact variant, 1, twice; ASCII again, 0; then three buffer layouts, the last of which — NULL rows that carry
bytes — ends on the general kernel, 2, under a flat output), "scanner" (GDV_NO_WAVE_SHAPE=1) and "selection" (UINT16 and
UINT32 projectors over four selections, and one that reaches the general kernel through NOTASCII).  Host batches on
the whole batch and on slices of 1, 63, 64, 65 and 2000 rows; device-resident batches on the whole batch."""
import json

import pyarrow as pa
import pytest

import string_shapes as R
from full_range_child import run_child

# time limits: twice the cold wall time of the slowest child of each mode on an MI355X (profiles/string_shapes.txt)
TIMEOUT = {"wave": 60, "scanner": 30, "selection": 80}


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("string_shapes")


def _write(case_dir, family, tag, full, expected):
    path = case_dir / ("%s_%s.arrow" % (family, tag.replace("/", "_")))
    if not path.exists():
        cols = {n: full.column(n) for n in R.SCHEMA.names}
        cols.update({"e%d" % i: e for i, e in enumerate(expected)})
        table = pa.table(cols)
        with pa.ipc.new_file(str(path), table.schema) as w:
            w.write_table(table)
    return str(path)


def _case(case_dir, family, mode):
    """Inputs and expected columns (from the reference) as Arrow files, the expressions and their grouping as JSON."""
    names = R.family_groups(family)
    specs, groups = [], []
    for name in names:
        groups.append(list(range(len(specs), len(specs) + len(R.group_specs(name)))))
        specs += [{"label": sp["label"], "tree": sp["tree"], "ret": sp["ret"], "ulps": None, "column": len(specs) + j} for j, sp in enumerate(R.group_specs(name))]

    def main_file(variant, nulls):
        tag = "%s/%s" % (variant, nulls)
        return tag, _write(case_dir, family, tag, R.batch(variant, nulls), [e for name in names for e in R.expected_columns(name, variant, nulls)])

    def layout_file(layout, variant):
        tag = "layout/%s/%s" % (layout, variant)
        return tag, _write(case_dir, family, tag, R.layout_batch(layout, variant), [e for name in names for e in R.expected_layout_columns(name, layout, variant)])
    case = {"family": "%s %s" % (family, mode), "mode": mode, "specs": specs, "groups": groups, "group_names": names, "files": []}
    if mode == "wave":
        case["files"] = [main_file(v, n) for v, n in R.MAIN_FILES] + [layout_file(l, v) for l in R.LAYOUTS[:2] for v in R.VARIANTS]
        case["null_bytes_files"] = [layout_file(R.LAYOUTS[2], v) for v in R.VARIANTS]
    elif mode == "scanner":
        case["files"] = [main_file("ascii", 0.1), main_file("multibyte", 0.1)]
    else:
        case["selection_files"] = [main_file("ascii", 0.0), main_file("ascii", 0.1), main_file("multibyte", 0.0)]
    path = case_dir / ("%s_%s.json" % (family, mode))
    path.write_text(json.dumps(case))
    return str(path)


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_wave_kernels_match_the_reference_on_every_boundary(case_dir, family):
    """Optimistic kernels, exact variant and back, the three layouts; host and device-resident batches."""
    run_child("string_shapes", _case(case_dir, family, "wave"), interpreted=False, timeout=TIMEOUT["wave"], extra_env=R.CHILD_MODES["wave"])


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_scanner_shaped_kernels_match_the_reference_on_every_boundary(case_dir, family):
    """The same projectors planned with GDV_NO_WAVE_SHAPE=1: the kernel every batch falls back to."""
    run_child("string_shapes", _case(case_dir, family, "scanner"), interpreted=False, timeout=TIMEOUT["scanner"], extra_env=R.CHILD_MODES["scanner"])


@pytest.mark.gpu
@pytest.mark.parametrize("family", R.FAMILIES)
def test_selection_mode_matches_the_reference_gathered_by_the_selection(case_dir, family):
    """UINT16 and UINT32 projectors: every row, every third row, the first and last row of each run, no row; an ASCII
    selection stays on the wave pair, one multi-byte row sends the batch to the general kernel."""
    run_child("string_shapes", _case(case_dir, family, "selection"), interpreted=False, timeout=TIMEOUT["selection"], extra_env=R.CHILD_MODES["selection"])


@pytest.mark.gpu
def test_a_per_row_pad_to_more_than_65536_characters_raises_on_the_row_that_needs_it():
    """The rule the corpus found undecided (PARITY.md): the device raises "invalid argument" for lpad(s, k) with k above
    65536 where the text is shorter than k, and pads to exactly 65536."""
    import gandiva_amd as gandiva
    from helpers import assert_bit_exact
    specs = [{"tree": R.F("lpad", "str", "s", "k"), "ret": "str"}, {"tree": R.F("rpad", "str", "s", "k", "t"), "ret": "str"}]
    proj = gandiva.make_projector(R.SCHEMA, R.build_expressions(gandiva, specs), None)

    def rows(s, k):
        return pa.RecordBatch.from_arrays([pa.array(s, pa.string()), pa.array(["é*"] * len(s), pa.string()), pa.array(s, pa.string()).cast(pa.binary()),
                                           pa.array(k, pa.int32())], schema=R.SCHEMA)
    quiet = rows(["a", "", None, "b", "x" * 70000, "日本"], [65536, 65537, 65537, None, 65537, 300])
    for g, w in zip(proj.evaluate(quiet), R.expected_of(specs, [c.to_pylist() for c in quiet.columns])):
        g.validate(full=True)
        assert_bit_exact(g, w, "pads at the limit")
    with pytest.raises(gandiva.GandivaError, match="invalid argument"):
        proj.evaluate(rows(["ab", "a"], [3, 65537]))
