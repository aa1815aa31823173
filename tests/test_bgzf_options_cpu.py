"""The BGZF options' host-side rules that need no GPU."""
import gzip

import pytest

from tests import inflate_cpu_lib as I


def test_sharded_runs_refuse_bgzf(tmp_path):
    from custom_porechop_abi_amd import shards
    with pytest.raises(ValueError):
        shards.trim_file_sharded(str(tmp_path / 'in.fastq'), str(tmp_path / 'out.fastq.gz'), 'fastq.gz',
                                 gzip_on_device=True, bgzf=True)


def test_only_bgzf_files_take_the_device_loader(tmp_path):
    from custom_porechop_abi_amd import misc
    text = b'@r1\nACGT\n+\n!!!!\n'
    files = {'plain.fastq': text, 'plain.fastq.gz': gzip.compress(text),
             'bgzf.fastq.gz': I.member(I.deflate_raw(text), text) + I.EOF_MARKER,
             'bgzf_extra.fastq.gz': I.member(I.deflate_raw(text), text, extra_before=b'XY\x01\x00q'), 'empty': b''}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        assert misc._starts_bgzf(str(tmp_path / name)) == name.startswith('bgzf')
    assert not misc._starts_bgzf(str(tmp_path / 'missing'))
    # the fallbacks load through the loader they always had, without a device
    for name in ('plain.fastq', 'plain.fastq.gz'):
        assert misc.load_batch(str(tmp_path / name), gunzip_device=0).n == 1
