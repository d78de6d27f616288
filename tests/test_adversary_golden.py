"""The host paths of Adversary.search and Adversary.shrink against tests/golden/adversary_paths.json
(made by tests/golden/make_adversary_golden.py on the commit named in the file): generations,
history, instance ids, the state of the random generator after the search and every counterexample,
bit for bit, with the oracle as evaluator."""
import pytest

from golden import make_adversary_golden as gen

GOLDEN = gen.load()


def test_golden_names_its_commit_and_every_case():
    for section, cases in (("host", gen.HOST_CASES), ("device", gen.DEVICE_CASES)):
        assert len(GOLDEN[section]["commit"]) == 40 and int(GOLDEN[section]["commit"], 16) >= 0
        assert (GOLDEN[section]["seed"], GOLDEN[section]["want"]) == (gen.SEED, gen.WANT)
        assert sorted(GOLDEN[section]["cases"]) == sorted(cases)
    found = {k: len(v["counterexamples"]) for k, v in GOLDEN["host"]["cases"].items()}
    assert all(found[k] == 2 for k in ("otr-safety", "fm-crash", "kses-crash", "otr-cap", "lv-mut")), found
    assert found["otr-live"] and found["lv-live"] and not found["otr-live-at"] and not found["ref-otr"]


@pytest.mark.parametrize("name", list(gen.HOST_CASES))
def test_host_search_replays_the_golden(name, oracle_mod):
    got, want = gen.record_host(name), GOLDEN["host"]["cases"][name]
    for k in sorted(set(got) | set(want)):
        assert got.get(k) == want.get(k), (name, k)
