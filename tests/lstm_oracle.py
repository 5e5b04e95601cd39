"""Plain-torch restatement of the LSTM tree refinement (/root/reference/models/danet/smpl_regressor.py:742-822) on torch's own
nn.LSTM, for the tests: the fp64 oracle of danet_densepose2smpl_amd.lstm_tree (run it on the CPU)."""
import torch

CHAINS = [(0, 3, 6, 9), (12, 15), (9, 13, 16, 18, 20, 22), (9, 14, 17, 19, 21, 23), (0, 1, 4, 7, 10), (0, 2, 5, 8, 11)]
NAMES = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')


def make_lstms(params, dtype=torch.float64):
    """params: five {name: tensor} dicts (nn.LSTM names) -> five nn.LSTM(128, 128, batch_first, bidirectional) holding them."""
    out = []
    for p in params:
        m = torch.nn.LSTM(128, 128, num_layers=1, batch_first=True, bidirectional=True).to(dtype)
        m.load_state_dict({k: v.detach().to(dtype) for k, v in p.items()})
        out.append(m)
    return out


def lstm_tree_ref(pos, lstms):
    """pos [B,24,128] -> cat(pos, pos) + chain outputs [B,24,256], as the reference combines them."""
    feats = {i: pos[:, i] for i in range(24)}
    refined = {}
    hidden = None
    for br, chain in enumerate(CHAINS):
        x = torch.stack([feats[j] for j in chain], dim=1)
        if br == 0:
            y, hidden = lstms[0](x)
        elif br == 1:
            y, _ = lstms[0](x, hidden)
        elif br in (2, 3):
            y, _ = lstms[br - 1](x, hidden)
        else:
            y, _ = lstms[br - 1](x)
        for i, j in enumerate(chain):
            if j == 0 and br != 0:
                continue
            refined[j] = y[:, i]
    return torch.stack([torch.cat([feats[i], feats[i]], 1) + refined[i] for i in range(24)], dim=1)
