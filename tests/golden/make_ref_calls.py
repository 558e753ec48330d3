#!/usr/bin/env python3
"""Regenerate tests/golden/ref_calls.{json,npz}: every call tests/test_oracle_vs_ref.py makes on the reference, with the
reference's answer (tests/helpers.py:RecordedRef).

Runs only where oracle/_ref/libdsc_ref.so exists (`make -C oracle ref`, from the reference's sources).  It runs each test
of that module against the reference build, so the recording is written only when they all pass.

    python tests/golden/make_ref_calls.py
"""
import inspect
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import tests.test_oracle_vs_ref as T  # noqa: E402
from tests.helpers import RecordedRef, RefRecording  # noqa: E402


def main():
    rec = RefRecording(empty=True)
    for name, f in inspect.getmembers(T, inspect.isfunction):
        if name.startswith('test_') and 'R' in inspect.signature(f).parameters:
            f(RecordedRef(name, recording=rec))
            print(f'{name}: {len(rec.calls[name])} calls')
    rec.save()
    size = sum(os.path.getsize(RefRecording.PATH + ext) for ext in ('.json', '.npz'))
    print(f'wrote {RefRecording.PATH}.json / .npz ({size / 1e3:.0f} kB)')


if __name__ == '__main__':
    main()
