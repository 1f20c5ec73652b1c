"""Child process of tests/test_gpu_resume.py: one seeded run of the streaming entry point with the command line given after the script name.
Test-only stop (read HERE, not in the product): SC_TEST_STOP_AFTER=N ends the run with exit status 17 when answer N + 1 is about to be
asked (SC_TEST_STOP_MODE=before, the default) or right after answer N + 1 has been appended to the results file but before its dialogue
turn and checkpoint are written (SC_TEST_STOP_MODE=after_write) - a process that died between two rounds / in the middle of one."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STOPPED = 17


class _Stop(Exception):
    pass


def main(argv):
    import numpy as np
    import torch
    import inference_streaming_longva_v2 as E
    stop_after, mode = int(os.environ.get("SC_TEST_STOP_AFTER", "0")), os.environ.get("SC_TEST_STOP_MODE", "before")
    if stop_after:
        real, calls = E.inference_thread_with_memory_and_dialogue_retrival_test, []

        def answer(*a, **k):
            calls.append(1)
            if len(calls) > stop_after and mode == "before":
                raise _Stop
            out = real(*a, **k)
            if len(calls) > stop_after:
                raise _Stop
            return out
        E.inference_thread_with_memory_and_dialogue_retrival_test = answer
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    try:
        E.run_inference(E.parse_args(argv))
    except _Stop:
        torch.cuda.synchronize()
        return STOPPED
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
