// Helper of profiles/measure_parse.py (no GPU code): the two host routes from a FASTQ file to the arrays a device batch is uploaded
// from, with the project's own readers.
//   old_fill    the cleaners' route: RecordBatch::fill (host/clean_common.h) into one std::string per line, the emptying of records
//               whose two strings differ in length, concat() of reads and qualities -- what bin/clean_lowqual does per batch; the
//               callback gets both planes and the offsets of every batch.
//   old_chunked ChunkedReadsFile (host/reads_io.h) with n_threads reader threads: bases only; the calling thread copies the
//               sequences of a window back to back (the programs pack them with several threads instead), the callback gets them
//               at the end of every window.
// Built by the script: g++ -O3 -shared -fPIC -I host -I include parse_old_route.cpp -lz -lpthread
#include "clean_common.h"
#include "reads_io.h"

extern "C" {

typedef void (*batch_cb)(const char *bases, const char *quals, const uint64_t *offsets, uint64_t n, uint64_t n_bytes);

// -> records, or -1 if the file cannot be opened
long long old_fill(const char *path, batch_cb cb)
{
	LineReader in(path, false);
	if (!in.ok()) return -1;
	RecordBatch batch;
	string bases, quals;
	vector<uint64_t> offsets;
	uint64_t raw_reads = 0, raw_bases = 0;
	for (bool more = true; more;) {
		more = batch.fill(in, raw_reads, raw_bases);
		for (size_t i = 0; i < batch.size(); i++)
			if (batch.reads[i].size() != batch.quals[i].size()) {
				batch.reads[i] = "";
				batch.quals[i] = "";
			}
		concat(batch.reads, bases, offsets);
		concat(batch.quals, quals, offsets);
		cb(bases.data(), quals.data(), offsets.data(), batch.size(), bases.size());
		batch.clear();
	}
	return (long long)raw_reads;
}

long long old_chunked(const char *path, int n_threads, batch_cb cb)
{
	ChunkedReadsFile m;
	if (!m.open(path)) return -1;
	string bases;
	vector<uint64_t> offsets(1, 0);
	long long reads = 0;
	const bool ok = m.for_each_read(1, n_threads,
	                                [&](const char *seq, size_t len) {
		                                bases.append(seq, len);
		                                offsets.push_back(bases.size());
	                                },
	                                [&]() {
		                                cb(bases.data(), nullptr, offsets.data(), offsets.size() - 1, bases.size());
		                                reads += (long long)offsets.size() - 1;
		                                bases.clear();
		                                offsets.assign(1, 0);
	                                });
	return ok ? reads : -1;
}
}
