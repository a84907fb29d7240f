"""CPU test of the chunk loop that the iterative fits share (``run_chunks`` in ``cca_zoo_amd/_utils/_resident.py``), with a
fake ``call`` in place of libccz."""

from cca_zoo_amd._utils._resident import run_chunks


def test_run_chunks_covers_total_and_ends_after_a_reported_stop():
    steps = []
    run_chunks(150, 64, lambda s: steps.append(s) or 0)
    assert steps == [64, 64, 22]                    # the steps sum to total, the last one short

    # the device stops inside chunk 1; as in libccz the call two chunks later is the first that is told
    told = []

    def call(s):
        told.append(s)
        return 1 if len(told) == 3 else 0

    run_chunks(10 * 64, 64, call)
    assert told == [64, 64, 64]                     # the first call that reports the stop is the last one

    steps = []
    run_chunks(5, 64, lambda s: steps.append(s) or 0)
    assert steps == [5]                             # total < chunk: one call
