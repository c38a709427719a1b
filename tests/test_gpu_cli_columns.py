"""phjoin --layout columns: both relations are split into key / payload columns
on the device before the join; the count and the aggregates are those of the
same command on tuples, and the JSON says which layout ran."""
import pytest

from test_gpu_cli import run_cli

pytestmark = pytest.mark.gpu

SIZES = ("--primary", "30000", "--secondary", "250000", "--seed", "4242")


@pytest.mark.parametrize("join", [("--join", "radix-partitioning", "--radix-bits", "8,8", "--hash", "murmur3"),
                                  ("--join", "no-partitioning")], ids=["radix", "nopart"])
@pytest.mark.parametrize("generate", ["host", "device"])
def test_cli_columns_count(tmp_path, join, generate):
    args = SIZES + join + ("--generate", generate)
    want, _ = run_cli(tmp_path, *args)
    got, _ = run_cli(tmp_path, *args, "--layout", "columns")
    assert int(got["device"]["matches"]) == int(want["device"]["matches"]) == 250_000
    assert got["device"]["layout"] == "columns" and want["device"]["layout"] == "tuples"
    assert list(got["results"]) == ["partition", "build", "probe"]


def test_cli_columns_aggregate(tmp_path):
    args = SIZES + ("--join", "radix-partitioning", "--radix-bits", "8,8", "--aggregate", "totals")
    want, _ = run_cli(tmp_path, *args)
    got, _ = run_cli(tmp_path, *args, "--layout", "columns")
    for k in ("pairs", "probe_matched", "sum_a", "sum_b", "sum_ab", "matches"):
        assert got["device"][k] == want["device"][k], k
    assert int(got["device"]["pairs"]) == 250_000
    assert got["device"]["layout"] == "columns"
