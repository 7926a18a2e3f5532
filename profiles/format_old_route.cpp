// Helper of profiles/measure_format.py (no GPU code): the text of an output file composed the way the cleaners compose it today.
//   old_compose  RecordBatch::fill (host/clean_common.h) reads a batch of records -- not timed --, then the loop of
//                RecordBatch::write puts every record's four lines into one std::string and hands the text over in pieces of 64 MiB
//                and more; where write() calls GzWriter::write the callback gets the piece (with DBGK_GZ=device that is the upload).
//                *compose_s is the time of the loop with the callbacks.
// Built by the script: g++ -O3 -shared -fPIC -I host -I include format_old_route.cpp -lz -lpthread
#include <chrono>

#include "clean_common.h"

extern "C" {

typedef void (*text_cb)(const char *text, uint64_t n_bytes);

// -> records, or -1 if the file cannot be opened
long long old_compose(const char *path, text_cb cb, double *compose_s)
{
	LineReader in(path, false);
	if (!in.ok()) return -1;
	RecordBatch batch;
	uint64_t raw_reads = 0, raw_bases = 0;
	double seconds = 0;
	for (bool more = true; more;) {
		more = batch.fill(in, raw_reads, raw_bases);
		const auto t0 = std::chrono::steady_clock::now();
		string text;
		for (size_t i = 0; i < batch.size(); i++) { // RecordBatch::write
			text += batch.heads[i]; text += '\n';
			text += batch.reads[i]; text += "\n+\n";
			text += batch.quals[i]; text += '\n';
			if (text.size() >= (64u << 20)) {
				cb(text.data(), text.size());
				text.clear();
			}
		}
		cb(text.data(), text.size());
		seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		batch.clear();
	}
	*compose_s = seconds;
	return (long long)raw_reads;
}
}
