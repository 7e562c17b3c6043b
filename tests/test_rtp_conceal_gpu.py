"""wmx_rtp_conceal_legs / wmx_rtp_reset_conceal / wmx_rtp_export_conceal (wmix_amd/csrc/rtp.hip, leg_plc.h) alone, through the Python
mirror, against tests/leg_plc_model.py: 70 legs -- more than one block of four, and no multiple of it -- 12 ticks of lists and rows
from the generator tests/test_leg_plc_host.py sweeps, so that every leg's history carries from tick to tick; some legs make no call in
some ticks, two are reset in mid-run.  Repaired rows, d_len_out, the exported history and the counter are compared after every tick.
Integers, np.array_equal."""
import numpy as np
import pytest

from conf_inputs import EINVAL
from leg_plc_model import LegsPlcModel, gen_case, pack, run_lengths

pytestmark = pytest.mark.gpu

N, T = 70, 12
SENTINEL = 0x5A5A


def script(seed, K, row):
    """-> per tick (pcm int16 [N, K, row], lens uint32 [N, K], words uint32 [N], the lists); one leg in five makes no call in a tick"""
    rng = np.random.default_rng(seed)
    ticks, runs = [], {1: 0, 2: 0, 3: 0}
    for _ in range(T):
        pcm, lens, lists = np.zeros((N, K, row), np.int16), np.zeros((N, K), np.uint32), []
        for g in range(N):
            if rng.integers(0, 5) == 0:
                lists.append([])
                continue
            calls, pcm[g], lens[g] = gen_case(rng, K, row=row)
            lists.append(calls)
            for r in run_lengths(calls, lens[g]):
                runs[min(r, 3)] += 1
        ticks.append((pcm, lens, np.array([pack(c) for c in lists], np.uint32), lists))
    assert all(v >= 20 for v in runs.values()), runs
    return ticks


def check_tick(snd, model, tick, cuda, what):
    import torch
    pcm, lens, words, lists = tick
    d_pcm, d_lens = torch.from_numpy(pcm).to(cuda), torch.from_numpy(lens.view(np.int32)).to(cuda)
    d_calls = torch.from_numpy(words.view(np.int32)).to(cuda)
    rows_out = torch.full((N, 4, 160), SENTINEL, dtype=torch.int16, device=cuda)
    lens_out = torch.full((N, 4), SENTINEL, dtype=torch.int32, device=cuda)
    snd.conceal_legs(d_pcm, d_lens, d_calls, rows_out, lens_out)
    want_rows, want_lens = model.tick(pcm, lens, lists)
    got_rows, got_lens = rows_out.cpu().numpy(), lens_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_lens, want_lens), (what, "d_len_out of legs", np.argwhere(got_lens != want_lens)[:8])
    made = np.repeat((want_lens == 320)[:, :, None], 160, axis=2)
    want_rows = np.where(made, want_rows, np.int16(SENTINEL))  # rows behind a leg's calls are not written
    assert np.array_equal(got_rows, want_rows), (what, "rows of (leg, call)", np.argwhere((got_rows != want_rows).any(2))[:8])
    got, want = snd.export_conceal(), model.export()
    assert np.array_equal(got["hist"], want["hist"]), (what, "history of legs", np.flatnonzero((got["hist"] != want["hist"]).any(1))[:8])
    assert np.array_equal(got["concealed"], want["concealed"]), (what, "concealed", got["concealed"], want["concealed"])
    # the call only reads what it is given
    assert np.array_equal(d_pcm.cpu().numpy(), pcm) and np.array_equal(d_lens.cpu().numpy().view(np.uint32), lens)
    assert np.array_equal(d_calls.cpu().numpy().view(np.uint32), words)
    return want


@pytest.mark.parametrize("K,row", [(1, 160), (3, 160), (3, 161)])  # rows of 161: every other row is off a 4-byte boundary
def test_every_tick_equals_the_model(cuda, K, row):
    from wmix_amd.rtp import RtpSenders
    ticks = script(40 + K + row, K, row)
    snd, model = RtpSenders(N), LegsPlcModel(N)
    first = snd.export_conceal()
    assert not first["hist"].any() and not first["concealed"].any()  # before any call: fresh
    some = [3, 66]  # one in the first block, one in the ragged last
    for t in range(T):
        if t == 6:
            before = model.export()
            assert before["hist"][some].any() and before["concealed"].sum() > 0
            snd.reset_conceal(some)
            model.reset(some)
            got, want = snd.export_conceal(), model.export()
            assert np.array_equal(got["hist"], want["hist"]) and np.array_equal(got["concealed"], want["concealed"])
            assert not want["hist"][some].any() and want["hist"].any()
        want = check_tick(snd, model, ticks[t], cuda, ("tick", t))
    assert want["concealed"].sum() >= 100 and (want["concealed"] > 0).sum() >= N // 2
    snd.reset_conceal()
    got = snd.export_conceal()
    assert not got["hist"].any() and not got["concealed"].any()
    snd.close()


def test_refusals_leave_state_and_outputs_alone(cuda, wmx):
    import torch
    from wmix_amd.rtp import RtpSenders
    K = 3
    ticks = script(11, K, 160)
    snd, model = RtpSenders(N), LegsPlcModel(N)
    for t in range(3):
        check_tick(snd, model, ticks[t], cuda, ("tick", t))
    stream = torch.cuda.current_stream().cuda_stream
    pcm, lens, words, _ = ticks[3]
    d_pcm, d_lens = torch.from_numpy(pcm).to(cuda), torch.from_numpy(lens.view(np.int32)).to(cuda)
    d_calls = torch.from_numpy(words.view(np.int32)).to(cuda)
    rows_out = torch.full((N, 4, 160), SENTINEL, dtype=torch.int16, device=cuda)
    lens_out = torch.full((N, 4), SENTINEL, dtype=torch.int32, device=cuda)
    before = snd.export_conceal()
    f = wmx.wmx_rtp_conceal_legs
    good = [snd._h, K, d_pcm.data_ptr(), K * 160, 160, d_lens.data_ptr(), d_calls.data_ptr(), rows_out.data_ptr(), lens_out.data_ptr(), stream]
    refused = []
    for at in (0, 2, 5, 6, 7, 8):  # every pointer NULL in turn
        refused.append(f(*[None if i == at else a for i, a in enumerate(good)]))
    for k in (0, 5, -1):
        refused.append(f(*[k if i == 1 else a for i, a in enumerate(good)]))
    refused.append(f(*[159 if i == 4 else a for i, a in enumerate(good)]))          # a row overlaps the next
    refused.append(f(*[K * 160 - 1 if i == 3 else a for i, a in enumerate(good)]))  # a leg overlaps the next
    refused.append(f(*[d_pcm.data_ptr() + 320 if i == 7 else a for i, a in enumerate(good)]))  # repaired rows inside their source
    bad = np.array([3, N], np.int32)
    refused.append(wmx.wmx_rtp_reset_conceal(snd._h, bad.ctypes.data, 2, stream))
    refused.append(wmx.wmx_rtp_reset_conceal(None, None, 0, stream))
    refused.append(wmx.wmx_rtp_export_conceal(None, None, None, stream))
    assert refused == [EINVAL] * len(refused), refused
    after = snd.export_conceal()
    assert np.array_equal(before["hist"], after["hist"]) and np.array_equal(before["concealed"], after["concealed"])
    assert (rows_out.cpu().numpy() == SENTINEL).all() and (lens_out.cpu().numpy() == SENTINEL).all()
    assert np.array_equal(d_pcm.cpu().numpy(), pcm)
    # either pointer of the export may be NULL
    concealed = np.zeros(N, np.uint32)
    assert wmx.wmx_rtp_export_conceal(snd._h, None, concealed.ctypes.data, stream) == 0 and np.array_equal(concealed, before["concealed"])
    assert wmx.wmx_rtp_export_conceal(snd._h, None, None, stream) == 0
    # and the handle still works
    check_tick(snd, model, ticks[3], cuda, "after the refusals")
    snd.close()
