"""Sequences by id, the parts that need no GPU: the tool exists and says how it is used, the binding knows the call, and
Index.sequences is still the number it has always been."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bwt-merge_amd", "csrc", "host")


def test_bwt_extract_builds_and_the_call_is_bound(bwtm):
    bwtm.build()
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "bwt_extract")
    assert os.path.exists(exe) and os.path.exists(os.path.join(HOST, "host_sequences_test"))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "Usage: bwt_extract [options] input output" in out.stderr
    for option in ("-g N", "-i format", "-f N", "-n N", "-m N"):
        assert option in out.stderr, option
    bound = {name: args for name, _, args in bwtm.capi.SYMBOLS}
    assert "bwtm_sequences_extract" in bound and len(bound["bwtm_sequences_extract"]) == 8
    assert hasattr(bwtm.capi.lib(), "bwtm_sequences_extract")
    assert bwtm.tune("extract_batch", 0) is None                        # the knob exists (an unknown key raises)


def test_sequence_count_is_an_int_that_can_be_called(bwtm):
    """Index.sequences keeps its meaning for everything that reads it as a number; calling it is the new Index.sequences(...)."""
    import json

    class FakeIndex:
        def extract_sequences(self, ids, first, count, max_len):
            return ("called", ids, first, count, max_len)

    n = bwtm.capi.SequenceCount(12, FakeIndex())
    assert isinstance(n, int) and n == 12 and n + 1 == 13 and n // 5 == 2 and "%d" % n == "12" and json.dumps({"n": n}) == '{"n": 12}'
    assert type(n + 0) is int and list(range(n))[-1] == 11 and hash(n) == hash(12)
    import copy
    import pickle
    assert type(pickle.loads(pickle.dumps(n))) is int and pickle.loads(pickle.dumps(n)) == 12 and copy.deepcopy(n) == 12
    assert n(first=3, count=4) == ("called", None, 3, 4, 0)
    assert n([5, 6], max_len=9) == ("called", [5, 6], 0, None, 9)
    assert callable(getattr(bwtm.Index, "extract_sequences"))
