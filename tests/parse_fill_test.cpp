// Test driver (no GPU): the records of the cleaners' record loop (host/clean_common.h: RecordBatch::fill) over one file.
// usage: parse_fill_test <file>; prints three lines per record, "<len>\t<text>" for the header, the read and the quality, and a
// last line "<raw reads>\t<raw bases>".
#include "clean_common.h"

int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	LineReader in(argv[1]);
	if (!in.ok()) return 3;
	RecordBatch batch;
	uint64_t raw_reads = 0, raw_bases = 0;
	for (bool more = true; more;) {
		more = batch.fill(in, raw_reads, raw_bases);
		for (size_t i = 0; i < batch.size(); i++)
			for (const string *s : {&batch.heads[i], &batch.reads[i], &batch.quals[i]}) {
				printf("%zu\t", s->size());
				fwrite(s->data(), 1, s->size(), stdout);
				putchar('\n');
			}
		batch.clear();
	}
	printf("%llu\t%llu\n", (unsigned long long)raw_reads, (unsigned long long)raw_bases);
	return 0;
}
