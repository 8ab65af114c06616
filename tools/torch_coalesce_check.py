"""Torch alone, no library: does `coalesce()` of a sparse COO tensor with wide fp32 values add duplicates right on this device?
(`profiles/r17a/torch_coalesce_wide_values.txt`; why `scone_amd/training.py` merges its sparse gradients itself.)"""
import torch
print(torch.__version__, torch.cuda.get_device_name(0))
torch.manual_seed(0)
for n, d, u in ((60, 768, 25), (60, 64, 25), (60, 256, 25), (60, 512, 25), (200, 768, 100), (60, 1024, 25)):
    ids = torch.sort(torch.randperm(n)[:u]).values.cuda()
    a, b = torch.randn(u, d, device="cuda"), torch.randn(u, d, device="cuda")
    sa = torch.sparse_coo_tensor(ids[None], a, (n, d), is_coalesced=True)
    sb = torch.sparse_coo_tensor(ids[None], b, (n, d), is_coalesced=True)
    got = (sa + sb).coalesce()
    want = a + b
    v = got.values()
    bad_cols = (v != want).any(dim=0).nonzero().reshape(-1)
    print(f"n={n} d={d} u={u}: nnz {v.shape[0]} wrong columns {bad_cols.numel()}" + (f" first {int(bad_cols[0])} all-zero there: {bool((v[:, bad_cols] == 0).all())}" if bad_cols.numel() else ""))
    sc = torch.sparse_coo_tensor(torch.cat([ids, ids])[None], torch.cat([a, b]), (n, d)).coalesce()
    print("   plain uncoalesced.coalesce(): wrong columns", int((sc.values() != want).any(dim=0).sum()))
